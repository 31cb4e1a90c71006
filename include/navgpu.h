/*
 * navgpu.h — C-ABI of the MI355X-native costmap + DWA hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch/ROS types.  The thin C++
 * plugin adapters (navigation_amd/plugin/, `nav_core::BaseLocalPlanner` and `costmap_2d::Layer`
 * subclasses) and the fleet harness (bench.py, tests) call exactly these entry points.  Every
 * entry point cites the reference interface it replaces (paths relative to the reference tree).
 *
 * Model: a *fleet* is N independent robot instances on one GPU, each with its own layered
 * costmap (master grid + layer grids) and DWA planner state, all of one grid size.  A single
 * robot is a fleet of 1.  Calls take an instance range [first, first+count) and are enqueued on
 * the fleet's HIP stream; `navgpu_sync` (or any *_results/_download call) waits for them.
 *
 * Conventions: return 0 on success, negative navgpu_status on error (no exceptions, like the
 * reference's bool / negative-cost error channel); the caller owns every buffer it passes.
 * There is NO CPU fallback: without a usable HIP device `navgpu_fleet_create` fails.
 *
 * Threading: every entry point that takes a fleet (or a navgpu_navfn / navgpu_amcl handle) holds that handle's
 * own recursive mutex for its whole body and makes the handle's GPU current on the calling thread,
 * so calls on ONE handle from several host threads are serialised inside the library: a
 * reconfigure (navgpu_planner_configure, navgpu_inflation_configure, navgpu_obstacle_configure,
 * navgpu_set_footprint ...) issued by a second thread while another is inside a stage / update /
 * cycle waits for that call to return, drains the stream before it frees or re-allocates a device
 * table, and a call that fails leaves the previous configuration in force.  This is the role of
 * DWAPlanner::configuration_mutex_ (dwa_local_planner/src/dwa_planner.cpp:55,301) and
 * InflationLayer::inflation_access_ (costmap_2d/plugins/inflation_layer.cpp:68,112,175).  What the
 * library cannot know is which calls form ONE control cycle: a caller that must not see a
 * reconfigure land between its stage and its cycle holds its own lock around the pair, as the
 * adapters do (navgpu::DWAPlannerROS::configuration_mutex_, the layers' gpu_access_ /
 * inflation_access_), next to the master-costmap mutex the reference already holds around both
 * virtual calls (costmap_2d/src/layered_costmap.cpp:83, move_base/src/move_base.cpp:947).
 * navgpu_fleet_destroy / navgpu_navfn_destroy / navgpu_amcl_destroy must not race any other call on the same handle.
 * Distinct handles are independent.  navgpu_last_error is per thread.
 */
#ifndef NAVGPU_H_
#define NAVGPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  NAVGPU_OK = 0,
  NAVGPU_ERR_INVALID = -1,   /* bad argument / range */
  NAVGPU_ERR_NO_DEVICE = -2, /* no HIP device, or kernels not loadable on it */
  NAVGPU_ERR_HIP = -3,       /* HIP runtime error (see navgpu_last_error) */
  NAVGPU_ERR_CAPACITY = -4,  /* input exceeds a capacity given at creation */
  NAVGPU_ERR_STATE = -5      /* call sequence violated (e.g. cycle before configure) */
} navgpu_status;

/* costmap_2d/include/costmap_2d/cost_values.h:42-45 */
#define NAVGPU_NO_INFORMATION 255
#define NAVGPU_LETHAL_OBSTACLE 254
#define NAVGPU_INSCRIBED_INFLATED_OBSTACLE 253
#define NAVGPU_FREE_SPACE 0

/* layer plugins present in an instance's LayeredCostmap, in the reference's plugin order
 * static -> obstacle|voxel -> inflation (costmap_2d/src/costmap_2d_ros.cpp:189-260) */
#define NAVGPU_LAYER_STATIC 1
#define NAVGPU_LAYER_OBSTACLE 2
#define NAVGPU_LAYER_VOXEL 4 /* replaces OBSTACLE: VoxelLayer derives from ObstacleLayer */
#define NAVGPU_LAYER_INFLATION 8

/* device-resident grids of an instance (navgpu_grid_upload / _download / _device) */
typedef enum {
  NAVGPU_GRID_MASTER = 0,     /* LayeredCostmap::costmap_, uint8 [size_y][size_x]                        */
  NAVGPU_GRID_STATIC = 1,     /* StaticLayer's costmap_, uint8                                           */
  NAVGPU_GRID_OBSTACLE = 2,   /* ObstacleLayer/VoxelLayer's costmap_, uint8                              */
  NAVGPU_GRID_VOXEL = 3,      /* VoxelGrid::data_, uint32 per column (voxel_grid.h:66-434)               */
  NAVGPU_GRID_PATH = 4,       /* MapGrid target_dist of path_costs_ (== alignment_costs_), uint32        */
  NAVGPU_GRID_GOAL = 5,       /* MapGrid target_dist of goal_costs_, uint32                              */
  NAVGPU_GRID_GOAL_FRONT = 6  /* MapGrid target_dist of goal_front_costs_, uint32                        */
} navgpu_grid_id;

typedef struct navgpu_fleet navgpu_fleet;
typedef struct navgpu_navfn navgpu_navfn;  /* a batch of global plans (NavFn section below) */

typedef struct {
  uint32_t n_instances;
  uint32_t size_x, size_y;  /* cells; Costmap2D::size_x_/size_y_ (costmap_2d.h:60-466)                   */
  double resolution;        /* m/cell                                                                   */
  int32_t layers;           /* NAVGPU_LAYER_* bitmask                                                   */
  int32_t track_unknown;    /* LayeredCostmap(track_unknown): master default 255 else 0 (layered_costmap.cpp:50-57) */
  int32_t device;           /* HIP device ordinal                                                       */
  uint32_t max_points;      /* capacity: cloud points per instance per update                           */
  uint32_t max_observations;/* capacity: observations per instance per update                           */
  uint32_t max_plan;        /* capacity: poses of the local plan handed to the planner                  */
  uint32_t max_footprint;   /* capacity: footprint polygon vertices                                     */
  uint32_t max_sim_steps;   /* capacity: trajectory points (ceil(sim_time/sim_granularity) or the
                               per-sample bound when discretize_by_time = 0)                            */
  int32_t keep_sample_costs;/* 1: keep every sample's total cost + status for navgpu_planner_samples.  The failure code of an
                               invalid sample (-2 .. -9) is computed only when it is kept: without this the product scoring launch
                               decides validity alone (same navgpu_plan_result, bit for bit)                */
  int32_t rolling_window;   /* LayeredCostmap(rolling_window): every update re-centres the grids on the robot
                               (Costmap2D::updateOrigin, costmap_2d.cpp:264-313; not with NAVGPU_LAYER_STATIC,
                               whose rolling branch needs tf)                                            */
} navgpu_fleet_desc;

/* One sensor observation of one instance — costmap_2d::Observation (observation.h:46-103):
 * origin_ (double xyz, global frame), cloud_ (float xyz, global frame), the two ranges.  This is
 * where the reference's own tests inject data (ObstacleLayer::addStaticObservation,
 * plugins/obstacle_layer.cpp:450-464; testing_helper.h:75-90). */
typedef struct {
  uint32_t instance;        /* absolute instance index                                                  */
  uint32_t first_point;     /* index of this cloud's first point in the packed points_xyz array         */
  uint32_t n_points;
  uint32_t flags;           /* bit0 marking, bit1 clearing                                              */
  double origin_x, origin_y, origin_z;
  double obstacle_range, raytrace_range;
} navgpu_observation;
#define NAVGPU_OBS_MARKING 1
#define NAVGPU_OBS_CLEARING 2

/* ObstacleLayer / VoxelLayer parameters (cfg/ObstaclePlugin.cfg:7-18, cfg/VoxelPlugin.cfg:10-15) */
typedef struct {
  int32_t enabled;
  int32_t footprint_clearing_enabled;
  int32_t combination_method; /* 0 overwrite, 1 max (costmap_layer.cpp:62-124) */
  int32_t z_voxels;           /* voxel only */
  double max_obstacle_height;
  double origin_z, z_resolution; /* voxel only */
  int32_t unknown_threshold;  /* voxel only, as configured (the +16-z_voxels of voxel_layer.cpp:89 is applied inside) */
  int32_t mark_threshold;     /* voxel only */
} navgpu_obstacle_params;

/* InflationLayer parameters (cfg/InflationPlugin.cfg:8-9) + the footprint's inscribed radius
 * (LayeredCostmap::getInscribedRadius, set through InflationLayer::onFootprintChanged) */
typedef struct {
  int32_t enabled;
  int32_t priority_queue_order; /* 0 (default): the order-independent windowed exact Euclidean transform - every cell takes
                                   the cost of its nearest LETHAL cell - on the parallel kernels.  1: InflationLayer::updateCosts
                                   as written (inflation_layer.cpp:226-293), byte for byte: a cell keeps the source carried by
                                   whichever neighbour std::priority_queue popped first (ties in libstdc++ heap order); one
                                   sequential walk per robot, far slower.  The two differ in ~6e-5 of the cells of a 400x400
                                   map at 1 % obstacles; 0 is never lower than 1 */
  double inflation_radius;
  double cost_scaling_factor;
  double inscribed_radius;
} navgpu_inflation_params;

/* base_local_planner::LocalPlannerLimits (local_planner_limits.h:44-124) + DWAPlannerConfig
 * (dwa_local_planner/cfg/DWAPlanner.cfg:15-36) + the plain params of DWAPlanner's ctor
 * (dwa_planner.cpp:131-181).  Field order is ABI. */
typedef struct {
  double max_trans_vel, min_trans_vel;
  double max_vel_x, min_vel_x, max_vel_y, min_vel_y;
  double max_rot_vel, min_rot_vel;
  double acc_lim_x, acc_lim_y, acc_lim_theta;
  double sim_time, sim_granularity, angular_sim_granularity, sim_period;
  double path_distance_bias, goal_distance_bias, occdist_scale;
  double forward_point_distance, cheat_factor;
  double oscillation_reset_dist, oscillation_reset_angle;
  int32_t vx_samples, vy_samples, vth_samples;
  int32_t use_dwa;            /* only 1 (DWA window, no continued acceleration) is accelerated   */
  int32_t discretize_by_time; /* SimpleTrajectoryGenerator::initialise(..., discretize_by_time)  */
  int32_t sum_scores;         /* ObstacleCostFunction::setSumScores                               */
  int32_t allow_unknown;      /* explicit (reference reads an uninitialised member)  */
  /* Which function computeNewPositions' unqualified cos(pos[2]) / sin(pos[2]) names for its FLOAT argument
   * (simple_trajectory_generator.cpp:253-260) depends on the reference's build, not on its source:
   *   0  ::cos(double) - only the C declarations in scope: the fork's own Kinetic / GCC 5 toolchain (default);
   *   1  the float overload - libstdc++ >= 6 puts std::cos(float) into the global namespace once <math.h> is in scope, and
   *      vel[0] * cos(pos[2]) becomes a float product (the M_PI_2 + pos[2] terms stay double).
   * INTEGRATION.md has a three-line probe that tells which one a workspace builds. */
  int32_t rollout_trig;
} navgpu_dwa_config;

/* Robot state for one planner cycle, already narrowed to float the way DWAPlanner::findBestPath
 * builds its Eigen::Vector3f pos / vel (dwa_planner.cpp:303-304). */
typedef struct {
  float pos[3];             /* x, y, yaw in the costmap's global frame */
  float vel[3];             /* vx, vy, vtheta                           */
  uint32_t plan_first;      /* first pose of this instance in the packed plan_xy array */
  uint32_t plan_count;      /* poses (>= 1); the transformed+pruned local plan          */
} navgpu_robot_state;

/* Result of DWAPlanner::findBestPath (dwa_planner.cpp:292-371) for one instance. */
typedef struct {
  int32_t best_index;       /* sample slot of the winner (x-outer, y, theta-inner order), -1 if none */
  int32_t n_samples;        /* sample slots generated this cycle                                      */
  int32_t n_scored;         /* slots the generator accepted                                           */
  int32_t n_valid;          /* slots with total cost >= 0                                             */
  int32_t n_points;         /* points of the winning trajectory                                       */
  uint32_t oscillation_flags;/* the 12 sticky flags after updateOscillationFlags (bit order: navgpu.h) */
  float xv, yv, thetav;     /* result_traj_.{xv_,yv_,thetav_}                                         */
  float reserved;
  double cost;              /* result_traj_.cost_ (-7 pre-set when nothing is valid)                  */
  double drive[3];          /* drive_velocities: (xv, yv, thetav) or zeros when cost < 0             */
} navgpu_plan_result;

/* oscillation flag bits (OscillationCostFunction members, oscillation_cost_function.cpp:81-97) */
#define NAVGPU_OSC_STRAFE_POS_ONLY (1u << 0)
#define NAVGPU_OSC_STRAFE_NEG_ONLY (1u << 1)
#define NAVGPU_OSC_STRAFING_POS (1u << 2)
#define NAVGPU_OSC_STRAFING_NEG (1u << 3)
#define NAVGPU_OSC_ROT_POS_ONLY (1u << 4)
#define NAVGPU_OSC_ROT_NEG_ONLY (1u << 5)
#define NAVGPU_OSC_ROTATING_POS (1u << 6)
#define NAVGPU_OSC_ROTATING_NEG (1u << 7)
#define NAVGPU_OSC_FORWARD_POS_ONLY (1u << 8)
#define NAVGPU_OSC_FORWARD_NEG_ONLY (1u << 9)
#define NAVGPU_OSC_FORWARD_POS (1u << 10)
#define NAVGPU_OSC_FORWARD_NEG (1u << 11)

/* per-sample status written when keep_sample_costs = 1 */
#define NAVGPU_SAMPLE_REJECTED 0 /* generateTrajectory returned false (simple_trajectory_generator.cpp:193-200,250) */
#define NAVGPU_SAMPLE_SCORED 1

/* ------------------------------------------------------------------------------------------ */
/* lifetime                                                                                   */
/* ------------------------------------------------------------------------------------------ */
const char* navgpu_version(void);
const char* navgpu_strerror(int status);
const char* navgpu_last_error(void); /* text of the last HIP failure on this thread */
int navgpu_device_count(void);

/* replaces: `new Costmap2DROS(...)` + plugin createInstance/initialize for the hot-path layers
 * (costmap_2d/src/costmap_2d_ros.cpp:63-167) and `DWAPlannerROS::initialize`
 * (dwa_local_planner/src/dwa_planner_ros.cpp:94-129), for n_instances robots at once. */
int navgpu_fleet_create(const navgpu_fleet_desc* desc, navgpu_fleet** out);
int navgpu_fleet_destroy(navgpu_fleet* fleet);
int navgpu_sync(navgpu_fleet* fleet);
void* navgpu_stream(navgpu_fleet* fleet); /* the fleet's hipStream_t */
/* Fault injection for tests (the counterpart of the reference's ObstacleLayer::addStaticObservation test hook,
 * costmap_2d/plugins/obstacle_layer.cpp:450-464): device allocations of this fleet larger than max_bytes fail with
 * NAVGPU_ERR_HIP from now on; 0 = no limit (default).  Used to check that a failed reconfigure leaves the previous
 * configuration in force. */
int navgpu_fleet_set_alloc_limit(navgpu_fleet* fleet, uint64_t max_bytes);

/* Costmap2D origin per instance (costmap_2d.h origin_x_/origin_y_); origins_xy = count x {x,y}.
 * replaces: LayeredCostmap::resizeMap origin arguments (layered_costmap.cpp:67-77) */
int navgpu_fleet_set_origin(navgpu_fleet* fleet, uint32_t first, uint32_t count, const double* origins_xy);
/* Costmap2D::getOriginX/Y — with a rolling window the origins move every navgpu_costmap_stage */
int navgpu_fleet_get_origin(navgpu_fleet* fleet, uint32_t first, uint32_t count, double* origins_xy);

/* raw grid access.  host buffers are count x size_y x size_x elements of the grid's type.
 * replaces: Costmap2D::getCharMap() (costmap_2d.cpp:187-190), VoxelGrid::getData() */
int navgpu_grid_upload(navgpu_fleet* fleet, int grid, uint32_t first, uint32_t count, const void* host);
int navgpu_grid_download(navgpu_fleet* fleet, int grid, uint32_t first, uint32_t count, void* host);
int navgpu_grid_device(navgpu_fleet* fleet, int grid, void** device_ptr, size_t* instance_stride_bytes);
/* replaces: Costmap2DPublisher::prepareGrid / the OccupancyGridUpdate window of publishCostmap
 * (costmap_2d/src/costmap_2d_publisher.cpp:57-74,103-115,146-156): cells [x0, xn) x [y0, yn) of the master grid
 * of one instance through the publisher's cost translation table (0, 1..98, 99, 100, -1), row-major into `out`
 * ((xn - x0) * (yn - y0) int8).  The message origin is the costmap origin (navgpu_fleet_get_origin). */
int navgpu_costmap_export(navgpu_fleet* fleet, uint32_t instance, uint32_t x0, uint32_t y0, uint32_t xn, uint32_t yn, int8_t* out);
/* Costmap2D::resetMaps() on the given grid (default value of that grid) */
int navgpu_grid_reset(navgpu_fleet* fleet, int grid, uint32_t first, uint32_t count);
/* replaces: Costmap2D::resetMap(x0, y0, xn, yn) (costmap_2d.cpp:93-99: rows [y0, yn), columns [x0, xn)) on
 * NAVGPU_GRID_MASTER or NAVGPU_GRID_OBSTACLE (a voxel layer's 2-D grid; its columns are untouched, as in the reference) */
int navgpu_grid_reset_window(navgpu_fleet* fleet, int grid, uint32_t first, uint32_t count, uint32_t x0, uint32_t y0, uint32_t xn, uint32_t yn);
/* replaces: CostmapLayer::resetBoundingBox(min, max) (costmap_layer.cpp:30-43; what Costmap2DROS::resetBoundingBox calls on
 * every CostmapLayer, costmap_2d_ros.cpp:574-611) on the obstacle / voxel layer: boxes = count x {min_x, min_y, max_x,
 * max_y} in world coordinates; the layer grid is reset inside (worldToMapEnforceBounds of both corners, resetMap) and the
 * box joins the bounds of the next navgpu_costmap_update / navgpu_obstacle_update_bounds (addExtraBounds / useExtraBounds). */
int navgpu_layer_reset_bounding_box(navgpu_fleet* fleet, uint32_t first, uint32_t count, const double* boxes);

/* ------------------------------------------------------------------------------------------ */
/* costmap layers                                                                             */
/* ------------------------------------------------------------------------------------------ */
/* replaces: StaticLayer::incomingMap (plugins/static_layer.cpp:167-228): occupancy is the
 * nav_msgs/OccupancyGrid int8 data of one map, interpreted with interpretValue (:149-163) on the
 * device and broadcast to [first, first+count).  The interpreted bytes are per instance; use_maximum is ONE setting of the
 * fleet (unlike the reference, where every costmap owns its StaticLayer): the value of the latest call, here or in
 * navgpu_static_set_rolling_map, holds for every robot from the next update on, whatever range that call named. */
int navgpu_static_set_map(navgpu_fleet* fleet, uint32_t first, uint32_t count, const int8_t* occupancy,
                          int32_t track_unknown_space, int32_t use_maximum, int32_t trinary_costmap,
                          int32_t lethal_cost_threshold, int32_t unknown_cost_value);

/* replaces: StaticLayer under a rolling window (plugins/static_layer.cpp:187-193 incomingMap resizes the layer only;
 * :262-283 updateBounds adds the layer's extent every cycle; :300-333 updateCosts maps every master cell of the update
 * window to world, through the map_frame <- global_frame transform, into the static map).  One static map (its own
 * size, resolution and origin) is shared by all robots of a rolling_window fleet created with NAVGPU_LAYER_STATIC. */
int navgpu_static_set_rolling_map(navgpu_fleet* fleet, const int8_t* occupancy, uint32_t size_x, uint32_t size_y, double resolution,
                                  double origin_x, double origin_y, int32_t track_unknown_space, int32_t use_maximum,
                                  int32_t trinary_costmap, int32_t lethal_cost_threshold, int32_t unknown_cost_value);
/* replaces: tf_->lookupTransform(map_frame_, global_frame_, ...) (static_layer.cpp:311): per robot 12 doubles, the
 * tf::Transform's 3x3 basis row-major followed by its origin.  Identity until set. */
int navgpu_static_set_transform(navgpu_fleet* fleet, uint32_t first, uint32_t count, const double* basis_origin);

/* replaces: ObstacleLayer::reconfigureCB / VoxelLayer::reconfigureCB */
int navgpu_obstacle_configure(navgpu_fleet* fleet, const navgpu_obstacle_params* params);
/* replaces: InflationLayer::setInflationParameters + onFootprintChanged + computeCaches
 * (plugins/inflation_layer.cpp:160-170,295-328,362-376).  The (R+2)^2 distance/cost tables are
 * built on the host in fp64 with libm exactly as the reference does, then uploaded. */
int navgpu_inflation_configure(navgpu_fleet* fleet, const navgpu_inflation_params* params);
/* footprint helpers, pure host functions (no fleet, no GPU).  xy = n x {x, y} in the robot frame.
 * replaces: costmap_2d::calculateMinAndMaxDistances (costmap_2d/src/footprint.cpp:41-67; DBL_MAX / 0 for n <= 2),
 * padFootprint (:138-147, in place), makeFootprintFromRadius (:150-167, 16 vertices). */
int navgpu_footprint_radii(const double* xy, uint32_t n, double* inscribed_radius, double* circumscribed_radius);
int navgpu_footprint_pad(double* xy, uint32_t n, double padding);
int navgpu_footprint_from_radius(double radius, double* xy16);
/* replaces: LayeredCostmap::setFootprint (layered_costmap.cpp:164-174) for [first,first+count).
 * footprint_xy = n_vertices x {x,y} in the robot frame.  Does NOT change inscribed_radius of the
 * inflation layer (pass it through navgpu_inflation_configure, as the adapter does). */
int navgpu_set_footprint(navgpu_fleet* fleet, uint32_t first, uint32_t count, const double* footprint_xy,
                         uint32_t n_vertices);

/* H2D staging of one update cycle's observations (host -> HBM).  poses = count x {x,y,yaw}.
 * replaces: ObstacleLayer::getMarkingObservations / getClearingObservations (:466-496) */
int navgpu_costmap_stage(navgpu_fleet* fleet, uint32_t first, uint32_t count, const double* robot_poses,
                         const navgpu_observation* observations, uint32_t n_observations,
                         const float* points_xyz, uint32_t n_points_total);
/* replaces: LayeredCostmap::updateMap(robot_x, robot_y, robot_yaw) (layered_costmap.cpp:79-150):
 * updateBounds of every layer (raytrace clearing, marking, footprint touch, inflation box union),
 * window reset, updateCosts of every layer — all on the device, boxes never visit the host. */
int navgpu_costmap_update(navgpu_fleet* fleet, uint32_t first, uint32_t count);
/* boxes = count x {x0, xn, y0, yn}: LayeredCostmap::getBounds (layered_costmap.h:131-137) */
int navgpu_costmap_bounds(navgpu_fleet* fleet, uint32_t first, uint32_t count, int32_t* boxes);

/* ---- the costmap update for a robot list.  The three calls above take [first, first + count); these take instances[0 .. n_robots),
 * strictly increasing, each < n_instances (NAVGPU_ERR_INVALID otherwise), as navgpu_planner_*_list do: the robots of a fleet whose
 * scan has just arrived, whichever they are, in one launch of each kernel; every robot outside the list stays byte for byte as it
 * was.  Per-robot arrays (robot_poses, boxes) are indexed by list position; navgpu_observation::instance stays a fleet index and
 * must be in the list (NAVGPU_ERR_INVALID).  Capacity checks are the range form's (NAVGPU_ERR_CAPACITY); a failed stage leaves
 * nothing staged.  Without a rolling window the calls leave what the range calls leave when they run contiguous run by
 * contiguous run over the same robots, bit for bit.
 * A rolling_window fleet takes these calls for ANY list (the range calls take it as a whole only): the origins and shifts of the
 * listed robots alone move, and the update shifts their grids alone, leaving the fleet's buffers where they are.  The pending
 * shift stays one per fleet: NAVGPU_ERR_STATE for a second stage before the update, for an update of another list than the one
 * staged, and for a range update behind a listed stage or the reverse. */
/* replaces: ObstacleLayer::getMarkingObservations / getClearingObservations (:466-496); rolling window: LayeredCostmap::updateMap
 * (layered_costmap.cpp:86-91) + Costmap2D::updateOrigin (costmap_2d.cpp:264-276) of the listed robots.  One packed upload of what
 * is in use and one scatter launch (k_cm_stage_scatter). */
int navgpu_costmap_stage_list(navgpu_fleet* fleet, uint32_t n_robots, const uint32_t* instances, const double* robot_poses,
                              const navgpu_observation* observations, uint32_t n_observations, const float* points_xyz,
                              uint32_t n_points_total);
/* replaces: LayeredCostmap::updateMap(robot_x, robot_y, robot_yaw) (layered_costmap.cpp:79-150) of the listed robots; rolling
 * window: Costmap2D::updateOrigin (costmap_2d.cpp:264-313) / VoxelLayer::updateOrigin (voxel_layer.cpp:385-440) of their grids first. */
int navgpu_costmap_update_list(navgpu_fleet* fleet, uint32_t n_robots, const uint32_t* instances);
/* boxes = n_robots x {x0, xn, y0, yn}: LayeredCostmap::getBounds (layered_costmap.h:131-137) */
int navgpu_costmap_bounds_list(navgpu_fleet* fleet, uint32_t n_robots, const uint32_t* instances, int32_t* boxes);

/* layer-granular calls for the costmap_2d::Layer adapters (layer.h:50-130).  boxes = count x
 * {min_i, min_j, max_i, max_j} as handed to Layer::updateCosts, or NULL to use the boxes the
 * last navgpu_costmap_update computed on the device.
 * replaces: InflationLayer::updateCosts (plugins/inflation_layer.cpp:172-266) */
int navgpu_inflate(navgpu_fleet* fleet, uint32_t first, uint32_t count, const int32_t* boxes);
/* replaces: ObstacleLayer::updateBounds / VoxelLayer::updateBounds on the staged observations;
 * bounds_inout = count x {min_x, min_y, max_x, max_y} */
int navgpu_obstacle_update_bounds(navgpu_fleet* fleet, uint32_t first, uint32_t count, double* bounds_inout);
/* replaces: ObstacleLayer::updateCosts (plugins/obstacle_layer.cpp:427-448): updateWithOverwrite /
 * updateWithMax (costmap_layer.cpp:62-124) of the layer grid into the master grid AS IT STANDS — what
 * the layers before this one wrote (upload it with navgpu_grid_upload) is kept; no window reset and no
 * static merge here, those belong to navgpu_costmap_update's fused LayeredCostmap::updateMap. */
int navgpu_obstacle_update_costs(navgpu_fleet* fleet, uint32_t first, uint32_t count, const int32_t* boxes);

/* ------------------------------------------------------------------------------------------ */
/* DWA local planner                                                                          */
/* ------------------------------------------------------------------------------------------ */
/* replaces: DWAPlanner::reconfigure (dwa_planner.cpp:52-116).  The eleven velocity / acceleration fields go into EVERY robot's limits
 * record (navgpu_planner_set_limits below): a caller who slowed one robot sets that robot's limits again after this call. */
int navgpu_planner_configure(navgpu_fleet* fleet, const navgpu_dwa_config* config);

/* base_local_planner::LocalPlannerLimits of ONE robot (local_planner_limits.h:47-65); field order is ABI */
typedef struct {
  double max_trans_vel, min_trans_vel;
  double max_vel_x, min_vel_x, max_vel_y, min_vel_y;
  double max_rot_vel, min_rot_vel;
  double acc_lim_x, acc_lim_y, acc_lim_theta;
  double xy_goal_tolerance, yaw_goal_tolerance;
  double trans_stopped_vel, rot_stopped_vel;
  int32_t prune_plan, reserved;
} navgpu_robot_limits;
/* replaces: LocalPlannerUtil::reconfigureCB (local_planner_util.cpp:59-71) of the robots [first, first+count), each of which owns
 * its LocalPlannerLimits in the reference (dwa_planner_ros.cpp:65-83), and MoveSlowAndClear::setRobotSpeed
 * (move_slow_and_clear.cpp:135-150,188-214) for the one robot that is recovering.  limits = count records.
 * One record feeds both halves, as the reference's one LocalPlannerLimits feeds DWAPlanner and LatchedStopRotateController: the
 * planner's (the eleven velocity / acceleration limits: sample windows, reject tests, continued acceleration,
 * updateOscillationFlags, the wavefront box) and the control cycle's (tolerances, stopped velocities, rot / acc limits, prune_plan).
 * Robots outside the range stay byte for byte as they were; sim_period, latch_xy_goal_tolerance and every other field of
 * navgpu_dwa_config stay the fleet's.  The fleet-wide calls keep their meaning: navgpu_planner_configure writes its eleven fields
 * into every robot's record, navgpu_local_planner_configure its fields into every robot's control half - set one robot's limits
 * again after either.  A fleet that never calls this behaves as if the call did not exist.
 * Takes effect with the robot's next staged cycle or probe (navgpu_planner_stage*, navgpu_planner_check_trajector*, the control
 * cycle), whose upload carries the record up: with two cycles in flight the queued cycle runs on the old limits, the next on the
 * new.  Inside what the fleet's scoring window and step capacity were planned for - the largest limits since the last
 * navgpu_planner_configure - the call allocates nothing and does not wait for the stream; beyond it, it re-plans the window and
 * image as navgpu_planner_configure does, all-or-nothing (NAVGPU_ERR_HIP, NAVGPU_ERR_CAPACITY when discretize_by_time = 0 needs
 * more than max_sim_steps: the previous limits stay in force).  NAVGPU_ERR_INVALID for a bad range, NULL or a non-finite field,
 * nothing changed; NAVGPU_ERR_STATE before the first navgpu_planner_configure.  Negative max_trans_vel / min_trans_vel /
 * min_rot_vel switch their test off, as in navgpu_dwa_config (the kernels' `>= 0` guards).
 * The legacy TrajectoryPlanner (navgpu_tp_config) has its own configuration and kernels and does not read these records. */
int navgpu_planner_set_limits(navgpu_fleet* fleet, uint32_t first, uint32_t count, const navgpu_robot_limits* limits);
/* replaces: LocalPlannerUtil::getCurrentLimits (local_planner_util.cpp:77-80) of the robots [first, first+count): what the calls
 * above left, the eleven velocity / acceleration fields from the planner's half */
int navgpu_planner_get_limits(navgpu_fleet* fleet, uint32_t first, uint32_t count, navgpu_robot_limits* limits);
/* replaces: DWAPlanner::setPlan (dwa_planner.cpp:204-207): resets the oscillation flags */
int navgpu_planner_set_plan(navgpu_fleet* fleet, uint32_t first, uint32_t count);
/* H2D staging of one control cycle (host -> HBM): robot states and the packed local plans
 * (plan_xy = n_plan_total x {x,y}).  Also performs DWAPlanner::updatePlanAndLocalCosts
 * (dwa_planner.cpp:240-286): nose goal and alignment on/off are evaluated here on the host in
 * fp64 libm, the same arithmetic the reference runs once per cycle. */
int navgpu_planner_stage(navgpu_fleet* fleet, uint32_t first, uint32_t count, const navgpu_robot_state* states,
                         const double* plan_xy, uint32_t n_plan_total);
/* A control cycle whose local plan has not changed since the last navgpu_planner_stage (move_base hands a new plan
 * at planner_frequency, the pose changes at controller_frequency): stages pose and velocity only, 24 B per robot
 * (pos_xyth, vel_xyth = count x 3 floats), and re-derives the nose goal / alignment switch of
 * DWAPlanner::updatePlanAndLocalCosts (dwa_planner.cpp:254-285) from the resident plan.  Needs a staged plan. */
int navgpu_planner_stage_poses(navgpu_fleet* fleet, uint32_t first, uint32_t count, const float* pos_xyth, const float* vel_xyth);
/* replaces: DWAPlanner::findBestPath (dwa_planner.cpp:292-371) =
 * SimpleTrajectoryGenerator::initialise + SimpleScoredSamplingPlanner::findBestTrajectory
 * (4 x MapGridCostFunction::prepare, rollout + six critics per sample, first-strict-minimum) +
 * OscillationCostFunction::updateOscillationFlags. */
int navgpu_planner_cycle(navgpu_fleet* fleet, uint32_t first, uint32_t count);
/* Bounded MapGrid wavefronts (no counterpart in the reference, which always runs computeTargetDistance over the whole
 * costmap, map_grid.cpp:262-310).  The critics read a MapGrid only at trajectory and forward points
 * (map_grid_cost_function.cpp:75-129), all inside a box around the robot of half edge
 * hypot(max |v_x|, max |v_y|) * sim_time + forward_point_distance; a level-synchronous wavefront has every cell it has
 * reached final, so the search of a cycle may stop once that box is settled.  enable = 1 (the default): it does, and the
 * grids of that cycle are exact inside the box and completed on demand before anything else reads them
 * (navgpu_grid_download / _device of the three MapGrids, navgpu_planner_cost_cloud, a checked trajectory that leaves
 * the box) — a request that comes after the costmap or the plan of that cycle has changed fails with
 * NAVGPU_ERR_STATE.  Robots within two such half edges of the end of their plan always get whole grids (the
 * stop-and-rotate controller keeps using them across cycles).  enable = 0: every cycle searches the whole grid, as
 * the reference does.  Planner results are identical either way. */
int navgpu_planner_set_bounded_map_grids(navgpu_fleet* fleet, int32_t enable);
/* Wavefront seed lists (no counterpart in the reference; results are identical either way).  enable = 1 (the default): a
 * cycle turns each robot's plan into the seed cells of its three MapGrids once (adjustPlanResolution + setTargetCells |
 * setLocalGoal, map_grid.cpp:135-258), ahead of the wavefronts, which then only scatter the cells.  enable = 0: every
 * wavefront walks the plan itself, as the launches outside a cycle always do.  Takes effect at the next cycle. */
int navgpu_planner_set_seed_lists(navgpu_fleet* fleet, int32_t enable);
/* Split image build (default: on).  Where a cycle scores with k_score_sweep and its wavefronts run in k_bfs_rows, the part of a
 * robot's scoring image that reads no distance grid (window, footprint screens, heading tables) is built by extra workgroups of
 * the wavefront launch itself, and k_score_prep_grids adds the path / goal screens behind it.  enable = 0: k_score_prep_tab
 * builds the whole image behind the wavefronts.  The results are the same bit for bit.  Takes effect at the next cycle. */
int navgpu_planner_set_split_prep(navgpu_fleet* fleet, int32_t enable);
/* Test hook: the seed cells a list holds, 1 .. 1024 (the default).  A (robot, grid) with more seed cells than that has no
 * list that cycle and its wavefront walks the plan.  NAVGPU_ERR_INVALID outside the range. */
int navgpu_planner_set_seed_list_capacity(navgpu_fleet* fleet, uint32_t cells);
/* introspection: the seed cells k_samples listed for the path / goal / goal_front wavefront of each instance the last time a
 * cycle with seed lists ran for it (counts = count x 3; duplicates count), 0xFFFFFFFF where the cells did not fit or no such
 * cycle has run. */
int navgpu_planner_seed_list_counts(navgpu_fleet* fleet, uint32_t first, uint32_t count, uint32_t* counts);
/* replaces: the MapGridCostFunction constructor arguments DWAPlanner never passes (map_grid_cost_function.h:64-69,
 * map_grid_cost_function.cpp:42-53, 75-129): aggregationType (0 Last - what DWAPlanner's four critics use -, 1 Sum,
 * 2 Product) and yshift (metres, sideways) of one critic: 0 path_costs_, 1 goal_costs_, 2 goal_front_costs_,
 * 3 alignment_costs_.  xshift stays DWAPlanner's (forward_point_distance for 2 and 3).  With any option set the scoring
 * launches take a general per-point step (no screen, no heading tables) and the wavefronts cover the whole map. */
int navgpu_planner_set_map_grid_options(navgpu_fleet* fleet, int32_t critic, int32_t aggregation, double yshift);
/* introspection: the number of wavefront levels the last cycle ran for the path / goal / goal_front grid of each instance
 * (levels = count x 3).  A whole-grid search runs until nothing new is reached, a bounded one stops earlier. */
int navgpu_planner_wavefront_levels(navgpu_fleet* fleet, uint32_t first, uint32_t count, uint32_t* levels);
/* introspection: the cell box {x0, x1, y0, y1} (inclusive) the last cycle's bounded wavefronts settled per instance
 * (boxes = count x 4); the whole map for an instance whose grids were searched whole */
int navgpu_planner_wavefront_boxes(navgpu_fleet* fleet, uint32_t first, uint32_t count, int32_t* boxes);
int navgpu_planner_results(navgpu_fleet* fleet, uint32_t first, uint32_t count, navgpu_plan_result* results);
/* Two control cycles in flight on the fleet's stream (no counterpart in the reference, whose cycle is a blocking call:
 * move_base.cpp:947 runs computeVelocityCommands to completion; an option of this library for callers that drive many
 * robots).  cycles = 2: navgpu_costmap_stage / navgpu_planner_stage of cycle k + 1 wait only until the copies out of
 * their pinned mirrors have run (a marker behind them), not for the stream, so cycle k + 1 can be handed over and queued
 * while cycle k runs; navgpu_planner_cycle then writes its results into the slot the cycle before it did not use, and
 * navgpu_planner_results_previous returns the results of the cycle BEFORE the latest queued one as soon as that cycle
 * has finished (NAVGPU_ERR_STATE when there is none).  navgpu_planner_results keeps its meaning: the latest queued cycle,
 * after the stream has drained.  With cycles = 2 a cycle covers the whole fleet (NAVGPU_ERR_STATE for a sub-range: the
 * result slot alternates per call).  cycles = 1 (default): every call as before.  The call itself drains the stream. */
int navgpu_planner_set_cycles_in_flight(navgpu_fleet* fleet, int32_t cycles);
int navgpu_planner_results_previous(navgpu_fleet* fleet, uint32_t first, uint32_t count, navgpu_plan_result* results);
/* winning trajectory of one instance: xyth = n_points x {x,y,theta}; returns n_points or <0 */
int navgpu_planner_trajectory(navgpu_fleet* fleet, uint32_t instance, double* xyth, uint32_t capacity_points);
/* every sample slot of one instance (needs keep_sample_costs): total cost with all critics summed
 * (no early-out; negative = the first failing critic's code) and NAVGPU_SAMPLE_* status */
int navgpu_planner_samples(navgpu_fleet* fleet, uint32_t instance, double* costs, int32_t* status,
                           float* velocities_xyz, uint32_t capacity);
/* replaces: DWAPlanner::checkTrajectory (dwa_planner.cpp:213-237) for one instance; uses the
 * staged state of that instance.  *ok = 1 when the single sample scores >= 0. */
int navgpu_planner_check_trajectory(navgpu_fleet* fleet, uint32_t instance, const float vel_samples[3], int32_t* ok);
/* replaces: a loop of DWAPlanner::checkTrajectory(pos, vel, vel_samples) calls (dwa_planner.cpp:213-237) over robots and samples.
 * instances: n_robots strictly increasing absolute robot indices (any subset of the fleet).  Robot k of the list owns the probes
 * probe_offsets[k] .. probe_offsets[k + 1] (probe_offsets[0] = 0, never decreasing); a robot without probes is left entirely alone,
 * its oscillation flags included.  Per (robot, probe) the contract is the single call's: the pose and velocity of the robot's last
 * navgpu_planner_stage / _stage_poses, the configuration, footprint, MapGrid options and rollout_trig in force; ordered on the
 * fleet's stream behind whatever is queued; returns when the answers are in the caller's arrays.  costs[p] is what
 * scoreTrajectory(traj, -1) returns - the full weighted sum, or the code of the first failing critic in the list - and
 * ok[p] = costs[p] >= 0 (costs may be NULL).  A probe the generator rejects is an empty trajectory: cost 0, ok 1 (the reference ignores
 * generateTrajectory's return value).  The oscillation critic sees cleared flags, and the flags of every robot with at least one
 * probe are zero afterwards (checkTrajectory resets them, :217).  One upload, one launch (k_check_traj) and one read-back for the
 * whole list; the answers go through a buffer of their own, so navgpu_planner_results / _samples / _trajectory still describe the
 * last cycle.  NAVGPU_ERR_INVALID: a null or malformed list (not increasing, out of range, decreasing offsets);
 * NAVGPU_ERR_STATE: before configure / stage.  The probe buffers grow on demand and are kept; when they cannot be allocated the
 * call fails with nothing launched and no flag reset. */
int navgpu_planner_check_trajectories(navgpu_fleet* fleet, uint32_t n_robots, const uint32_t* instances,
                                      const uint32_t* probe_offsets /* n_robots + 1 */, const float* vel_samples /* 3 per probe */,
                                      int32_t* ok /* per probe */, double* costs /* per probe, may be NULL */);
/* The planner cycle for a robot LIST: navgpu_planner_stage / _stage_poses / _cycle / _results for the robots instances[0 .. n_robots),
 * strictly increasing absolute robot indices, each < n_instances, 1 <= n_robots <= n_instances (the conventions of
 * navgpu_planner_check_trajectories); anything else is NAVGPU_ERR_INVALID with nothing changed.  Per-robot arrays are indexed by
 * list position k.  In a fleet the robots inside their goal tolerance are scattered among the driving ones; a list costs one
 * launch of each kernel of the cycle whatever it looks like, where contiguous ranges cost a stage, a cycle and a wait per run.
 * Contract: the listed robots end up as if every contiguous run of the list had been handed to the range calls in turn - nothing
 * in the cycle reduces across robots, so that is bit equality - and every robot outside the list keeps result, trajectory,
 * sample costs, oscillation flags, MapGrids, wavefront levels and boxes and trajectory-cloud records as they were.
 * replaces (per listed robot), as the range forms do:
 *   _stage_list        DWAPlanner::updatePlanAndLocalCosts (dwa_planner.cpp:240-286); states[k].plan_first / plan_count index
 *                      plan_xy as in navgpu_planner_stage.  Same validation, all or nothing (plan_count 0: NAVGPU_ERR_INVALID, above
 *                      max_plan: NAVGPU_ERR_CAPACITY).  One packed upload - the records and only the poses in use - and one scatter
 *                      kernel (k_stage_scatter).
 *   _stage_poses_list  the pose-only stage of a cycle whose plans have not changed (pos_xyth, vel_xyth = n_robots x 3 floats);
 *                      NAVGPU_ERR_STATE naming the robot when a listed robot has no staged plan.
 *   _cycle_list        dwaComputeVelocityCommands' planner call (dwa_planner_ros.cpp:176-247) = DWAPlanner::findBestPath
 *                      (dwa_planner.cpp:292-371) per listed robot.  NAVGPU_ERR_STATE before configure / stage, and with two cycles
 *                      in flight (navgpu_planner_set_cycles_in_flight(f, 2) takes whole-fleet range cycles only).  An enabled
 *                      trajectory-cloud robot gets its terms pass when it is in the list, and only then.
 *   _results_list      one wait; results[k] is the result of instances[k]. */
int navgpu_planner_stage_list(navgpu_fleet* fleet, uint32_t n_robots, const uint32_t* instances, const navgpu_robot_state* states,
                              const double* plan_xy, uint32_t n_plan_total);
int navgpu_planner_stage_poses_list(navgpu_fleet* fleet, uint32_t n_robots, const uint32_t* instances, const float* pos_xyth,
                                    const float* vel_xyth);
int navgpu_planner_cycle_list(navgpu_fleet* fleet, uint32_t n_robots, const uint32_t* instances);
int navgpu_planner_results_list(navgpu_fleet* fleet, uint32_t n_robots, const uint32_t* instances, navgpu_plan_result* results);
/* replaces: DWAPlanner::getCellCosts (dwa_planner.cpp:185-202) over the whole map + MapGridVisualizer::publishCostCloud
 * (base_local_planner/src/map_grid_visualizer.cpp:55-83): the cost cloud of one instance from the grids of its last
 * cycle.  points = up to `capacity` x {x, y, z, path_cost, goal_cost, occ_cost, total_cost} (MapGridCostPoint), in the
 * reference's order (cx outer, cy inner, cells for which getCellCosts returns false skipped).  Returns the
 * number of points of the full cloud. */
int navgpu_planner_cost_cloud(navgpu_fleet* fleet, uint32_t instance, float* points, uint32_t capacity);
/* replaces: the publish_traj_pc parameter (dwa_planner.cpp:160-163), per robot.  An enabled robot's navgpu_planner_cycle runs a
 * terms pass behind its scoring launch and before the winner is selected (the reference builds the cloud before
 * updateOscillationFlags, dwa_planner.cpp:321-357): every sample slot is scored again and the raw value of each critic, the
 * first failing critic and the point count are kept.  Robots that are not enabled run the launches they ran before.  At most
 * NAVGPU_TRAJ_CLOUD_MAX_ROBOTS robots of a fleet are enabled at once (NAVGPU_ERR_INVALID beyond that; the records live in
 * memory that exists only for them); NAVGPU_ERR_STATE with two cycles in flight (navgpu_planner_set_cycles_in_flight, which in
 * turn refuses 2 while a robot is enabled); NAVGPU_ERR_CAPACITY when max_sim_steps points do not fit a workgroup's LDS. */
#define NAVGPU_TRAJ_CLOUD_MAX_ROBOTS 16
int navgpu_planner_set_trajectory_cloud(navgpu_fleet* fleet, uint32_t first, uint32_t count, int32_t enable);
/* replaces: the trajectory_cloud of DWAPlanner::findBestPath (dwa_planner.cpp:318-348): every point of every explored
 * trajectory whose cost is >= 0, slot by slot and within a slot point by point.  points = up to `capacity` x
 * {x, y, z, path_cost, goal_cost, occ_cost, total_cost} (MapGridCostPoint): x = (float)p_x, y = (float)p_y, z = 0,
 * path_cost = (float)p_th, total_cost = (float)cost.  The reference assigns these five fields of an uninitialised local
 * (dwa_planner.cpp:323, 339-343) and leaves goal_cost and occ_cost indeterminate; they are 0 here.
 * reference_costs = 1: the cost is Trajectory::cost_ as SimpleScoredSamplingPlanner::scoreTrajectory left it
 * (simple_scored_sampling_planner.cpp:50-79, 111-127): the in-order sum of the critic terms, cut at the first failing critic
 * or behind the first term that takes it above the best cost of the slots before it - so most costs are partial sums, and a
 * slot whose later critic would have failed can be a member.  reference_costs = 0: the cost is the full sum and the members
 * are the slots whose full sum is >= 0 (independent of the order of the slots).
 * Returns the number of points of the full cloud; points beyond `capacity` are not written and nothing is written behind the
 * last point; points = NULL with capacity = 0 counts only.  The cloud is built at this call from the terms of the robot's last
 * cycle.  NAVGPU_ERR_STATE: the robot is not enabled, no cycle has run since it was, or it was staged or reconfigured after
 * that cycle; NAVGPU_ERR_INVALID: bad instance, or points == NULL with a capacity. */
int navgpu_planner_trajectory_cloud(navgpu_fleet* fleet, uint32_t instance, int32_t reference_costs, float* points, uint32_t capacity);
/* one sample slot of the last cycle of an enabled robot (no counterpart as a call: what scoreTrajectory,
 * simple_scored_sampling_planner.cpp:50-79, works through for all_explored[i]) */
typedef struct {
  double critic[5];      /* raw (unscaled) value of obstacle, goal_front, alignment, path, goal (dwa_planner.cpp:167-173 after the
                            oscillation critic); the failing critic holds its code; NaN where the reference never evaluated the
                            critic: scale 0, or behind the first failing critic */
  double cost_full;      /* every term summed; the failing critic's code; -1 for a slot the generator rejected */
  double cost_ref;       /* Trajectory::cost_ in the reference's flow (early-out against the incumbent) */
  int32_t first_fail;    /* 0 oscillation, 1 obstacle ... 5 goal, 6 none */
  int32_t status;        /* NAVGPU_SAMPLE_* */
  int32_t n_points;
  int32_t member;        /* 1: the slot's points are in the cloud (reference_costs = 1) */
  uint32_t point_offset; /* index of its first point in that cloud (the points of the members before it) */
  uint32_t reserved;
} navgpu_sample_terms;
/* out = up to `capacity` slots in slot order; returns the number of slots.  Errors as for navgpu_planner_trajectory_cloud. */
int navgpu_planner_sample_terms(navgpu_fleet* fleet, uint32_t instance, navgpu_sample_terms* out, uint32_t capacity);
/* OscillationCostFunction state access (persists across cycles per instance) */
int navgpu_planner_get_oscillation(navgpu_fleet* fleet, uint32_t first, uint32_t count, uint32_t* flags,
                                   float* prev_stationary_pos_xyz);
int navgpu_planner_set_oscillation(navgpu_fleet* fleet, uint32_t first, uint32_t count, const uint32_t* flags,
                                   const float* prev_stationary_pos_xyz);

/* ------------------------------------------------------------------------------------------ */
/* DWAPlannerROS control cycle: the steps around findBestPath         */
/* ------------------------------------------------------------------------------------------ */
/* Host-side mirror, free of ROS types, of DWAPlannerROS::setPlan / computeVelocityCommands /
 * isGoalReached (dwa_local_planner/src/dwa_planner_ros.cpp:130-158,176-300), of
 * LocalPlannerUtil::getLocalPlan (base_local_planner/src/local_planner_util.cpp:105-123) with
 * goal_functions.cpp's transformGlobalPlan / prunePlan / getGoalPose / stopped (:69-174,175-255) and of
 * LatchedStopRotateController (src/latched_stop_rotate_controller.cpp:37-273).  Poses are (x, y, yaw)
 * triples; the tf lookup is replaced by an optional planar plan->global transform handed in by the
 * caller (identity when NULL).  tf's own 3-D arithmetic and the `angles` package are not part of the
 * reference tree: their formulas are restated (angles::normalize_angle: fmod form), parity unpinned. */
typedef struct {
  double xy_goal_tolerance, yaw_goal_tolerance;  /* LocalPlannerLimits (local_planner_limits.h)            */
  double rot_stopped_vel, trans_stopped_vel;
  double max_rot_vel, min_rot_vel;
  double acc_lim_x, acc_lim_y, acc_lim_theta;    /* limits.getAccLimits()                                   */
  double sim_period;                             /* DWAPlanner::getSimPeriod()                              */
  int32_t prune_plan;                            /* LocalPlannerLimits::prune_plan                          */
  int32_t latch_xy_goal_tolerance;               /* ~/latch_xy_goal_tolerance                               */
} navgpu_local_limits;

typedef struct {
  double pose[3];      /* costmap_ros_->getRobotPose(): x, y, yaw in the costmap's global frame             */
  double odom_vel[3];  /* OdometryHelperRos: twist.linear.x, twist.linear.y, twist.angular.z               */
  int32_t have_pose;   /* 0: getRobotPose failed -> computeVelocityCommands returns false                   */
  int32_t reserved;
} navgpu_robot_input;

typedef enum {
  NAVGPU_BRANCH_NONE = 0,     /* returned before dispatching (no pose, no plan, empty local plan)           */
  NAVGPU_BRANCH_DWA = 1,      /* dwaComputeVelocityCommands                                                 */
  NAVGPU_BRANCH_STOP = 2,     /* stop-rotate: stopWithAccLimits                                             */
  NAVGPU_BRANCH_ROTATE = 3,   /* stop-rotate: rotateToGoal                                                  */
  NAVGPU_BRANCH_AT_GOAL = 4,  /* stop-rotate: goal orientation reached, zero command                        */
  NAVGPU_BRANCH_ROLLOUT = 5   /* TrajectoryPlannerROS: tc_->findBestPath's drive velocities (navgpu_tp_ros_*) */
} navgpu_branch;

typedef struct {
  double cmd_vel[3];          /* geometry_msgs::Twist linear.x, linear.y, angular.z                         */
  int32_t ok;                 /* return value of computeVelocityCommands                                    */
  int32_t branch;             /* navgpu_branch                                                              */
  int32_t local_plan_points;  /* poses of the transformed + pruned plan handed to updatePlanAndLocalCosts   */
  int32_t trajectory_points;  /* points of the published local plan (winning trajectory; 0 unless DWA ok)   */
} navgpu_cmd_result;

/* transformGlobalPlan (goal_functions.cpp:88-174) followed, when `prune` is set, by prunePlan
 * (:69-86) on a plan of n (x, y, yaw) triples.  dist_threshold = max(size_x, size_y) * resolution / 2
 * (:119-120).  Writes the local plan to out_xyyaw (capacity poses), its length to *n_out and the number
 * of poses prunePlan erased from the FRONT OF THE STORED GLOBAL PLAN to *n_erased (it erases both plans in
 * lockstep from their beginnings).  Pure host function: needs no fleet and no GPU.
 * Returns NAVGPU_OK, NAVGPU_ERR_INVALID (n == 0: "Received plan with zero length") or NAVGPU_ERR_CAPACITY. */
int navgpu_local_plan_window(const double* plan_xyyaw, uint32_t n, const double pose[3], const double* plan_to_global,
                             double dist_threshold, int32_t prune, double* out_xyyaw, uint32_t capacity,
                             uint32_t* n_out, uint32_t* n_erased);
/* angles::shortest_angular_distance(from, to) as restated here (exposed for the parity tests) */
double navgpu_shortest_angular_distance(double from, double to);

/* LocalPlannerUtil::reconfigureCB limits + LatchedStopRotateController parameters, for the whole fleet: the control cycle's half
 * of every robot's limits record (navgpu_planner_set_limits changes one robot's) */
int navgpu_local_planner_configure(navgpu_fleet* fleet, const navgpu_local_limits* limits);
/* DWAPlannerROS::setPlan: stores the global plan of one instance (n (x, y, yaw) triples in the plan's own
 * frame), clears the goal-tolerance latch and resets the oscillation flags.  plan_to_global = NULL: the
 * plan is already expressed in the costmap's global frame. */
int navgpu_local_planner_set_plan(navgpu_fleet* fleet, uint32_t instance, const double* plan_xyyaw, uint32_t n,
                                  const double* plan_to_global);
/* DWAPlannerROS::computeVelocityCommands for instances [first, first+count): getLocalPlan ->
 * updatePlanAndLocalCosts -> isPositionReached ? computeVelocityCommandsStopRotate (checkTrajectory on
 * the GPU as the obstacle check, MapGrids NOT refreshed: the reference does not call prepare() there)
 * : dwaComputeVelocityCommands (navgpu_planner_cycle over the instances on that branch). */
int navgpu_local_planner_compute_velocity_commands(navgpu_fleet* fleet, uint32_t first, uint32_t count,
                                                   const navgpu_robot_input* in, navgpu_cmd_result* out);
/* DWAPlannerROS::isGoalReached -> LatchedStopRotateController::isGoalReached */
int navgpu_local_planner_is_goal_reached(navgpu_fleet* fleet, uint32_t first, uint32_t count,
                                         const navgpu_robot_input* in, int32_t* reached);
/* the stored global plan of one instance after pruning; returns its length (poses) or < 0 */
int navgpu_local_planner_get_plan(navgpu_fleet* fleet, uint32_t instance, double* xyyaw, uint32_t capacity);

/* ---- Device-resident global plans: LocalPlannerUtil::getLocalPlan as a kernel (k_plan_window) ----
 * A robot's global plan may live on the device instead of in the host vector navgpu_local_planner_set_plan keeps.  The store
 * holds n_instances x max_global_plan (x, y, yaw) records; per robot the host keeps where the live part of its slot starts and
 * how long it is (prunePlan's erase from the front moves the start, no pose is moved), the planar plan -> global transform and
 * whether the robot's plan is resident at all.  navgpu_local_planner_compute_velocity_commands then runs getLocalPlan for the
 * resident robots of its range as one kernel launch and reads one navgpu_local_window (plus the window's last point and the
 * goal pose) per robot back; no plan pose crosses the bus in either direction.  Robots whose plan came through
 * navgpu_local_planner_set_plan keep the host path; one range may hold both kinds.
 * navgpu_planner_stage on a resident robot replaces the window of that one cycle as it does for any robot (the caller hands
 * it a local plan); the next navgpu_local_planner_compute_velocity_commands derives the window from the store again.
 * navgpu_planner_stage_poses after a resident cycle behaves as after a host-path cycle: a cycle whose local plan comes out empty
 * (nothing within reach, or everything pruned) stages nothing, and the robot's window of the cycle before stays on the device.
 * One difference: when the call returns NAVGPU_ERR_CAPACITY because a resident robot's window does not fit, the resident robots
 * of the range whose windows did fit already hold this cycle's window on the device (the host path stages none then); the
 * library's record of every such window's length and last point follows, so a later navgpu_planner_stage_poses is consistent
 * with it.  Stored plans are pruned only for the robots before the failing one, as on the host path. */
typedef enum {
  NAVGPU_LOCAL_WINDOW_OK = 0,
  NAVGPU_LOCAL_WINDOW_NONE = 1,      /* no window was taken: no pose, no plan, or "Received plan with zero length"        */
  NAVGPU_LOCAL_WINDOW_CAPACITY = 2   /* the window has more than max_plan poses; the stored plan was left as it was        */
} navgpu_local_window_status;
typedef struct {
  int32_t first_index;  /* index in the stored plan (before the erase) of the first pose within reach, -1: none (also: host path) */
  int32_t n_window;     /* poses transformGlobalPlan took, the one that leaves the reach included                            */
  int32_t n_erased;     /* poses prunePlan erased from the front of both plans                                               */
  int32_t n_local;      /* n_window - n_erased: the local plan's length                                                      */
  int32_t remaining;    /* length of the stored plan after the erase                                                         */
  int32_t status;       /* navgpu_local_window_status                                                                        */
} navgpu_local_window;
typedef enum { NAVGPU_PLAN_FAMILY_GLOBAL_PLANNER = 0, NAVGPU_PLAN_FAMILY_NAVFN_ROS = 1 } navgpu_plan_family;

/* replaces: the storage behind LocalPlannerUtil::setPlan's global_plan_ (base_local_planner/src/local_planner_util.cpp:87-103)
 * for a fleet.  Allocates the store, or resizes it (resident plans are carried over; one that is longer than the new size:
 * NAVGPU_ERR_CAPACITY).  A call that fails leaves the previous store, its plans included, in force.  A fleet that never calls
 * this allocates nothing for it. */
int navgpu_local_planner_reserve_plans(navgpu_fleet* fleet, uint32_t max_global_plan);
/* replaces: DWAPlannerROS::setPlan (dwa_local_planner/src/dwa_planner_ros.cpp:130-140) -> LocalPlannerUtil::setPlan
 * (local_planner_util.cpp:87-103) for robots [first, first+count) at once: plan k is poses_xyyaw[offsets[k] .. offsets[k+1])
 * as (x, y, yaw) triples in its own frame, plan_to_global = count x (x, y, yaw) transforms or NULL (plans already in the global
 * frame).  One upload; goal-tolerance latches cleared, oscillation flags reset.  A plan of zero poses is stored as such (the
 * cycle then reports "Received plan with zero length": ok 0, NAVGPU_BRANCH_NONE).  A plan longer than max_global_plan:
 * NAVGPU_ERR_CAPACITY, nothing stored for any robot.  NAVGPU_ERR_STATE without a store or a configured local planner. */
int navgpu_local_planner_set_plans(navgpu_fleet* fleet, uint32_t first, uint32_t count, const double* poses_xyyaw,
                                   const uint32_t* offsets, const double* plan_to_global);
/* replaces: move_base handing planner_->makePlan's result to tc_->setPlan (move_base/src/move_base.cpp:576-600, 888) for plans
 * [nav_first, nav_first+count) of a NavFn handle and robots [fleet_first, fleet_first+count), without the plans leaving the
 * device: the emit kernel of navgpu_global_planner_plans / navgpu_navfn_ros_plans (family: navgpu_plan_family) writes plan
 * nav_first + k into the slot of robot fleet_first + k.  State checks as in those calls (NAVGPU_ERR_STATE when a plan's last
 * maker was not of that family).  A plan that was not made (n_poses 0) is not adopted: the robot keeps its previous plan and
 * adopted_out[k] = 0, as move_base keeps the controller's plan when makePlan fails.  A plan longer than max_global_plan is not
 * adopted either, and the call returns NAVGPU_ERR_CAPACITY AFTER adopting the others (adopted_out says which).  Both handles
 * must live on the same device (NAVGPU_ERR_INVALID).  The two streams are ordered with events.  adopted_out may be NULL. */
int navgpu_local_planner_adopt_plans(navgpu_fleet* fleet, uint32_t fleet_first, navgpu_navfn* nav, uint32_t nav_first,
                                     uint32_t count, int32_t family, const double* plan_to_global, int32_t* adopted_out);
/* replaces: publishGlobalPlan(transformed_plan) (dwa_local_planner/src/dwa_planner_ros.cpp:166-168, 278, 292): the transformed, pruned plan of the instance's last cycle as (x, y, yaw) triples; returns its length or < 0.
 * Works for host-path and resident robots (for the latter the poses are read from the store and transformed on the host). */
int navgpu_local_planner_local_plan(navgpu_fleet* fleet, uint32_t instance, double* xyyaw, uint32_t capacity);
/* replaces: what LocalPlannerUtil::getLocalPlan (local_planner_util.cpp:105-123) did in the last cycle, per robot:
 * transformGlobalPlan's window and prunePlan's erase (goal_functions.cpp:69-174) as counts. */
int navgpu_local_planner_windows(navgpu_fleet* fleet, uint32_t first, uint32_t count, navgpu_local_window* out);

/* ------------------------------------------------------------------------------------------ */
/* Legacy base_local_planner::TrajectoryPlanner ("Trajectory Rollout")              */
/* ------------------------------------------------------------------------------------------ */
/* The second nav_core::BaseLocalPlanner of the reference (TrajectoryPlannerROS).  Same structure as the
 * DWA path - two MapGrid wavefronts (path_map_ with the cells under the robot's own footprint marked
 * within_robot, goal_map_), a rollout per velocity sample with footprint and grid look-ups - but fp64
 * state with acceleration-limited velocities, a different sample enumeration and a sequential, stateful
 * selection (in-place rotation / strafing / backing up with oscillation and escape flags).  The GPU rolls
 * out every candidate sample of createTrajectories; the host replays the reference's selection over the
 * per-sample results.  heading_scoring (headingDiff's line-of-sight scan over the plan, :372-386) and simple_attractor
 * (:310-315) are options of the same rollout. */
typedef struct {
  double acc_lim_x, acc_lim_y, acc_lim_theta;
  double sim_time, sim_granularity, angular_sim_granularity;
  double pdist_scale, gdist_scale, occdist_scale; /* after the meter_scoring multiplication, if any */
  double heading_lookahead, oscillation_reset_dist, escape_reset_dist, escape_reset_theta;
  double max_vel_x, min_vel_x, max_vel_th, min_vel_th, min_in_place_vel_th;
  double backup_vel;                              /* escape_vel */
  double sim_period;
  double heading_scoring_timestep;                /* BaseLocalPlanner.cfg: 0.1 (TrajectoryPlannerROS's own param default: 0.8) */
  double y_vels[8];
  int32_t n_y_vels;
  int32_t vx_samples, vtheta_samples;
  int32_t holonomic_robot, dwa, allow_unknown;
  int32_t heading_scoring, simple_attractor;
} navgpu_tp_config;

/* TrajectoryPlanner members that persist between cycles (trajectory_planner.h:290-300) */
#define NAVGPU_TP_STUCK_LEFT (1u << 0)
#define NAVGPU_TP_STUCK_RIGHT (1u << 1)
#define NAVGPU_TP_ROTATING_LEFT (1u << 2)
#define NAVGPU_TP_ROTATING_RIGHT (1u << 3)
#define NAVGPU_TP_STUCK_LEFT_STRAFE (1u << 4)
#define NAVGPU_TP_STUCK_RIGHT_STRAFE (1u << 5)
#define NAVGPU_TP_STRAFE_LEFT (1u << 6)
#define NAVGPU_TP_STRAFE_RIGHT (1u << 7)
#define NAVGPU_TP_ESCAPING (1u << 8)
typedef struct {
  uint32_t flags;
  uint32_t reserved;
  double prev_x, prev_y, escape_x, escape_y, escape_theta;
} navgpu_tp_state;

typedef struct {
  double xv, yv, thetav, cost;   /* the returned Trajectory                                             */
  double drive[3];               /* drive_velocities (zeros when cost < 0)                              */
  int32_t n_points;              /* points of that trajectory                                           */
  int32_t n_samples;             /* generateTrajectory calls the reference would have made this cycle   */
  int32_t best_sample;           /* index of the winner among them (call order)                         */
  int32_t reserved;
} navgpu_tp_result;

/* one generateTrajectory call as the reference makes it (call order) */
typedef struct {
  double vx, vy, vtheta;         /* the sample                                                          */
  double cost;                   /* traj.cost_: >= 0, -1 (off map / collision) or -2 (no path to goal)  */
  int32_t n_points;
  int32_t reserved;
} navgpu_tp_sample;

/* replaces: TrajectoryPlanner::TrajectoryPlanner / reconfigure (trajectory_planner.cpp:58-172); footprint
 * from navgpu_set_footprint.  Also sizes the per-robot sample buffers. */
int navgpu_tp_configure(navgpu_fleet* fleet, const navgpu_tp_config* config);
/* replaces: TrajectoryPlanner::updatePlan(new_plan, compute_dists) (:474-500) for one instance; plan_xy =
 * n x {x, y} in the costmap's global frame. */
int navgpu_tp_update_plan(navgpu_fleet* fleet, uint32_t instance, const double* plan_xy, uint32_t n, int32_t compute_dists);
/* replaces: TrajectoryPlanner::findBestPath (:908-984) for instances [first, first+count): pos / vel of
 * `states` are the Eigen::Vector3f the reference builds (plan fields ignored). */
int navgpu_tp_find_best_path(navgpu_fleet* fleet, uint32_t first, uint32_t count, const navgpu_robot_state* states,
                             navgpu_tp_result* results);
/* the winning trajectory's points (x, y, theta); returns n_points or < 0 */
int navgpu_tp_trajectory(navgpu_fleet* fleet, uint32_t instance, double* xyth, uint32_t capacity_points);
/* the generateTrajectory calls of the last cycle of one instance, in the reference's call order */
int navgpu_tp_samples(navgpu_fleet* fleet, uint32_t instance, navgpu_tp_sample* samples, uint32_t capacity);
/* replaces: TrajectoryPlanner::scoreTrajectory / checkTrajectory (:502-531) against the current grids */
int navgpu_tp_score_trajectory(navgpu_fleet* fleet, uint32_t instance, const double pose[3], const double vel[3],
                               const double vel_samples[3], double* cost);
int navgpu_tp_get_state(navgpu_fleet* fleet, uint32_t first, uint32_t count, navgpu_tp_state* states);
int navgpu_tp_set_state(navgpu_fleet* fleet, uint32_t first, uint32_t count, const navgpu_tp_state* states);
/* replaces: TrajectoryPlanner::updatePlan(new_plan, compute_dists) (trajectory_planner.cpp:474-500) for robots [first, first+count):
 * plan k = plans_xy[offsets[k] .. offsets[k+1]) as {x, y} pairs in the costmap's global frame (offsets never decrease).  Per robot the
 * effects of navgpu_tp_update_plan; with compute_dists the plans of the range go up together, ONE wavefront launch covers the range and
 * the call waits once.  A plan longer than max_plan: NAVGPU_ERR_CAPACITY, nothing changed for any robot. */
int navgpu_tp_update_plans(navgpu_fleet* fleet, uint32_t first, uint32_t count, const double* plans_xy,
                           const uint32_t* offsets /* count + 1 */, int32_t compute_dists);
/* replaces: a loop of TrajectoryPlanner::scoreTrajectory / checkTrajectory calls (trajectory_planner.cpp:502-531) over robots and
 * probes, against the robots' current grids.  The conventions of navgpu_planner_check_trajectories: instances = n_robots strictly
 * increasing robot indices, robot k owns the probes probe_offsets[k] .. probe_offsets[k + 1] (probe_offsets[0] = 0, never decreasing), a
 * robot without probes is left alone; an empty list (n_robots = 0) is no work and no error.  A probe is 9 doubles: pose x, y, theta,
 * velocity x, y, theta, sample x, y, theta.  costs[p] is scoreTrajectory's value (>= 0, -1 off the map or in collision, -2 no path to
 * the goal), ok[p] = costs[p] >= 0 is checkTrajectory's (ok may be NULL).  One upload, one launch (k_tp_probe: a wave per probe, a lane
 * per step; bit-equal to the single call) and one read-back for the whole list, ordered on the fleet's stream.  The probes go through
 * buffers of their own, grown on demand and kept: navgpu_tp_samples / _trajectory and the results of the last navgpu_tp_find_best_path
 * still describe that cycle (the single call, navgpu_tp_score_trajectory, borrows the robot's sample slot 0 and start state).
 * NAVGPU_ERR_INVALID: a null or malformed list (not increasing, out of range, decreasing offsets) or a probe value that is not finite;
 * NAVGPU_ERR_STATE, nothing launched: before navgpu_tp_configure, or simple_attractor with an empty plan on a listed robot that has
 * probes. */
int navgpu_tp_score_trajectories(navgpu_fleet* fleet, uint32_t n_robots, const uint32_t* instances,
                                 const uint32_t* probe_offsets /* n_robots + 1 */, const double* probes /* 9 per probe */,
                                 double* costs /* per probe */, int32_t* ok /* per probe, may be NULL */);
/* navgpu_tp_update_plans / navgpu_tp_find_best_path for a robot list, with the conventions of navgpu_planner_*_list: instances = n_robots
 * strictly increasing robot indices, each < n_instances (else NAVGPU_ERR_INVALID); plans, offsets, states and results go by position in
 * the list; an empty list (n_robots = 0) is no work and no error.  What a call leaves - results, navgpu_tp_samples / _trajectory /
 * _get_state, both MapGrids - is bit-equal to the range calls run contiguous run by contiguous run over the same robots, and every robot
 * outside the list stays byte for byte as it was.  The cost does not depend on how the robots lie in the fleet: the list, ONE packed
 * block that holds only what is in use (plan points, samples, the cells under the robots, start states) and one launch that spreads it;
 * each kernel of the range call once (k_free_bits, k_tp_within, the wavefronts, k_tp_rollout) with the list where that passes `first`;
 * the listed robots' results packed on the device and read in one copy; the second pass's winners the same way up.
 * Errors are checked before anything is uploaded or launched, nothing changed for any robot: NAVGPU_ERR_STATE before navgpu_tp_configure
 * and (find_best_path) for simple_attractor with an empty plan on a listed robot; NAVGPU_ERR_CAPACITY for a plan longer than max_plan. */
int navgpu_tp_update_plans_list(navgpu_fleet* fleet, uint32_t n_robots, const uint32_t* instances, const double* plans_xy,
                                const uint32_t* offsets /* n_robots + 1 */, int32_t compute_dists);
int navgpu_tp_find_best_path_list(navgpu_fleet* fleet, uint32_t n_robots, const uint32_t* instances, const navgpu_robot_state* states,
                                  navgpu_tp_result* results);

/* ---- TrajectoryPlannerROS control cycle for a fleet (base_local_planner/src/trajectory_planner_ros.cpp:283-597) ----
 * Host-side mirror, free of ROS types, of TrajectoryPlannerROS::setPlan / computeVelocityCommands / stopWithAccLimits / rotateToGoal /
 * checkTrajectory / scoreTrajectory / isGoalReached round the navgpu_tp_* core, as navgpu_local_planner_* mirrors DWAPlannerROS: poses are
 * (x, y, yaw) triples, the tf lookup is an optional planar plan -> global transform, transformGlobalPlan + prunePlan are
 * navgpu_local_plan_window (the goal_functions.cpp code TrajectoryPlannerROS calls at :386-393).  The class needs tf and ROS and cannot be
 * compiled against the reference tree here: parity of these entry points is unpinned in the sense of the DWAPlannerROS mirror above.
 * Acceleration limits, max_vel_th, min_vel_th, min_in_place_vel_th and sim_period are those of navgpu_tp_config. */
typedef struct {
  double xy_goal_tolerance, yaw_goal_tolerance;         /* 0.10, 0.05 (trajectory_planner_ros.cpp:118-119)   */
  double rot_stopped_velocity, trans_stopped_velocity;  /* 1e-2, 1e-2 (:97-98)                               */
  int32_t latch_xy_goal_tolerance;                      /* 0 (:126)                                          */
  int32_t prune_plan;                                   /* 1 (:116)                                          */
} navgpu_tp_ros_params;
/* replaces: the parameter reads of TrajectoryPlannerROS::initialize / reconfigureCB that belong to the ROS class itself.
 * NAVGPU_ERR_STATE before navgpu_tp_configure. */
int navgpu_tp_ros_configure(navgpu_fleet* fleet, const navgpu_tp_ros_params* params);
/* replaces: TrajectoryPlannerROS::setPlan (:355-370) for robots [first, first+count): plan k is poses_xyyaw[offsets[k] .. offsets[k+1])
 * as (x, y, yaw) triples in its own frame, plan_to_global = count x (x, y, yaw) or NULL.  Clears xy_tolerance_latch_ and reached_goal_;
 * rotating_to_goal_ stays as it is (the reference does not reset it there). */
int navgpu_tp_ros_set_plans(navgpu_fleet* fleet, uint32_t first, uint32_t count, const double* poses_xyyaw, const uint32_t* offsets,
                            const double* plan_to_global);
/* replaces: TrajectoryPlannerROS::computeVelocityCommands (:372-526) for robots [first, first+count), line by line:
 * 1. the window per robot (navgpu_local_plan_window, dist_threshold = max(size_x, size_y) * resolution / 2; the stored plan is erased in
 *    lockstep when prune_plan is set).  No pose, a zero-length plan or an empty window: ok 0, NAVGPU_BRANCH_NONE.  A window longer than
 *    max_plan: NAVGPU_ERR_CAPACITY for the call, as in navgpu_local_planner_compute_velocity_commands.
 * 2. the goal is the LAST POSE OF THE TRANSFORMED WINDOW (:411-419), not the end of the global plan.  Position reached:
 *    xy_tolerance_latch_ || distance <= xy_goal_tolerance; the latch is set only with latch_xy_goal_tolerance.
 * 3. reached and |shortest_angular_distance(yaw, goal_th)| <= yaw_goal_tolerance: zero command, rotating_to_goal_ and the latch cleared,
 *    reached_goal_ set, ok 1, NAVGPU_BRANCH_AT_GOAL; no updatePlan / findBestPath for this robot.
 * 4. every other robot with a window: updatePlan(transformed_plan) + findBestPath - also the robots whose position is reached (:443-444:
 *    the reference refreshes the grids and advances the planner's oscillation / escape state there and discards the result).  ONE
 *    updatePlan and ONE findBestPath for all of them: navgpu_tp_update_plans + navgpu_tp_find_best_path when they form one contiguous
 *    run, else navgpu_tp_update_plans_list + navgpu_tp_find_best_path_list - robots of step 3 or without a window cost no launch.
 * 5. position reached: stopWithAccLimits' candidate while !rotating_to_goal_ && !stopped(odom) (NAVGPU_BRANCH_STOP), else
 *    rotating_to_goal_ = true and rotateToGoal's (NAVGPU_BRANCH_ROTATE).  All candidates are checked in ONE navgpu_tp_score_trajectories
 *    call behind step 4, so they see this cycle's grids, within_robot included.  Invalid: zero command, ok 0.
 * 6. the others: NAVGPU_BRANCH_ROLLOUT, cmd_vel = drive velocities, ok = cost >= 0, trajectory_points = the winner's length (0 when
 *    the cost is negative); the points stay readable through navgpu_tp_trajectory.
 * local_plan_points = the window's length. */
int navgpu_tp_ros_compute_velocity_commands(navgpu_fleet* fleet, uint32_t first, uint32_t count, const navgpu_robot_input* in,
                                            navgpu_cmd_result* out);
/* replaces: TrajectoryPlannerROS::isGoalReached (:590-597): reached_goal_, the flag the last cycle set */
int navgpu_tp_ros_is_goal_reached(navgpu_fleet* fleet, uint32_t first, uint32_t count, int32_t* reached);
/* replaces: a loop of TrajectoryPlannerROS::checkTrajectory / scoreTrajectory(vx, vy, vtheta, update_map) calls (:528-588) over robots
 * (instances strictly increasing, in[k] the input of robot instances[k]) and velocity samples (3 doubles per probe, probe_offsets as in
 * navgpu_tp_score_trajectories).  With update_map the listed robots first get updatePlan({pose}, true) - the planner's plan and final
 * goal become the robot's pose, as in the reference - in ONE navgpu_tp_update_plans_list; then one navgpu_tp_score_trajectories call with
 * pose and vel = odom_vel.  A robot without a pose: cost -1.0, ok 0, neither updated nor probed.  ok may be NULL. */
int navgpu_tp_ros_check_trajectories(navgpu_fleet* fleet, uint32_t n_robots, const uint32_t* instances, const navgpu_robot_input* in,
                                     const uint32_t* probe_offsets, const double* vel_samples, int32_t update_map, double* costs,
                                     int32_t* ok);
/* global_plan_ of one instance after pruning; returns its length (poses) or < 0 */
int navgpu_tp_ros_get_plan(navgpu_fleet* fleet, uint32_t instance, double* xyyaw, uint32_t capacity);
/* replaces: publishPlan(transformed_plan, g_plan_pub_) (:468, :499, :523): the window of the instance's last cycle; its length or < 0 */
int navgpu_tp_ros_transformed_plan(navgpu_fleet* fleet, uint32_t instance, double* xyyaw, uint32_t capacity);
/* Pure host function, needs no fleet: the velocity candidate of stopWithAccLimits (:283-290, rotate = 0; pose and goal_th unused) or of
 * rotateToGoal (:312-337, rotate = 1) as vel_samples_out = {vx, vy, vth}.  NAVGPU_ERR_INVALID for a NULL argument. */
int navgpu_tp_ros_candidate(const navgpu_tp_config* config, int32_t rotate, const double pose[3], const double odom_vel[3],
                            double goal_th, double vel_samples_out[3]);

/* ------------------------------------------------------------------------------------------ */
/* Footprint-cost queries, rotate_recovery::RotateRecovery, carrot_planner::CarrotPlanner       */
/* ------------------------------------------------------------------------------------------ */
/* replaces: WorldModel::footprintCost(x, y, theta, footprint_spec) -> CostmapModel::footprintCost
 * (base_local_planner/include/base_local_planner/world_model.h:65-86, base_local_planner/src/costmap_model.cpp:50-142)
 * called directly - "is this footprint legal at these poses" - against the RESIDENT master grid, origin and footprint
 * (navgpu_set_footprint) of every robot in [first, first+count).  query_counts = count run lengths (0 is legal);
 * poses_xyth = sum(query_counts) x {x, y, theta} doubles in the world frame, robot after robot.  costs_out = one double per
 * query: -1.0 when the centre or an oriented vertex is off the map, or an outline cell is LETHAL, or NO_INFORMATION with
 * allow_unknown = 0; else the largest cell cost over the outline (LineIterator cells of every edge, the closing one
 * included).  With fewer than 3 vertices: the centre cell's cost, and INSCRIBED fails too (:60-67).  allow_unknown is explicit
 * (CostmapModel derives it from the costmap's default value, :45-48).  first_illegal_out (or NULL) = per robot
 * the index within its run of the first query with a negative cost, -1 when there is none; found on the device.
 * A pose that is not finite is NAVGPU_ERR_INVALID, here as in the two calls below.
 * Ordered on the fleet's stream behind whatever was queued before (a navgpu_costmap_update, say); returns when the results
 * are on the host.  NAVGPU_ERR_STATE while a staged rolling-window origin has not been applied by an update yet. */
int navgpu_footprint_cost(navgpu_fleet* fleet, uint32_t first, uint32_t count, const uint32_t* query_counts, const double* poses_xyth,
                          int32_t allow_unknown, double* costs_out, int32_t* first_illegal_out);

/* RotateRecovery's parameters (rotate_recovery/src/rotate_recovery.cpp:60-66): sim_granularity 0.017, and from
 * ~/TrajectoryPlannerROS acc_lim_th 3.2, max_rotational_vel 1.0, min_in_place_rotational_vel 0.4, yaw_goal_tolerance 0.10.
 * (frequency, 20.0, is the caller's: one navgpu_rotate_recovery_step per tick.)  allow_unknown: what
 * CostmapModel(*local_costmap_->getCostmap()) derives from the costmap's default value (:68, costmap_model.cpp:45-48),
 * explicit here. */
typedef struct {
  double sim_granularity;
  double acc_lim_th;
  double max_rotational_vel;
  double min_in_place_rotational_vel;
  double yaw_goal_tolerance;
  int32_t allow_unknown;
  int32_t reserved;
} navgpu_rotate_recovery_params;
/* capacity: headings of one robot's sweep in one step.  A sweep covers less than 2 pi, so sim_granularity must be at least
 * 2 pi / (NAVGPU_ROTATE_RECOVERY_MAX_SWEEP - 1) (about 0.00154 rad) */
#define NAVGPU_ROTATE_RECOVERY_MAX_SWEEP 4096

/* the locals of RotateRecovery::runBehavior that live across iterations of its loop (:100-104), per robot */
typedef struct {
  double start_offset;  /* 0 - normalize_angle(yaw) at the first step of a run                                            */
  int32_t got_180;
  int32_t started;      /* 0: the next step begins a run (sets start_offset, clears got_180); cleared again by DONE / BLOCKED */
  int32_t swept;        /* out: headings the last step checked - the whole sweep, or up to and including the illegal one   */
  int32_t reserved;
} navgpu_rotate_recovery_state;

typedef enum {
  NAVGPU_ROTATE_RUNNING = 0, /* cmd_wz published, loop continues (:137-152)                                               */
  NAVGPU_ROTATE_DONE = 1,    /* cmd_wz published, then got_180 && current_angle >= -tolerance (:148-150)                  */
  NAVGPU_ROTATE_BLOCKED = 2  /* a swept heading has negative footprint cost: the early return of :123-126, cmd_wz = 0    */
} navgpu_rotate_status;

/* replaces: RotateRecovery::initialize's parameter reads (:55-66).  NAVGPU_ERR_INVALID for a sim_granularity that is not
 * positive, NAVGPU_ERR_CAPACITY for one below the bound above; a call that fails changes nothing. */
int navgpu_rotate_recovery_configure(navgpu_fleet* fleet, const navgpu_rotate_recovery_params* params);
/* replaces: one pass of the while(n.ok()) body of RotateRecovery::runBehavior (:105-153) for every robot of
 * [first, first+count).  poses_xyth = count x {x, y, yaw}: local_costmap_->getRobotPose.  The headings yaw + sim_angle, with
 * sim_angle grown by repeated += sim_granularity from 0 while < dist_left (:117-129), of all robots are checked in one
 * k_footprint_cost launch; cmd_wz_out = min(max(sqrt(2 * acc_lim_th * dist_left), min_in_place_rotational_vel),
 * max_rotational_vel) (:131-135), status_out = navgpu_rotate_status.  The caller publishes cmd_wz and steps again after
 * 1 / frequency while the status is RUNNING.  angles::normalize_angle: the fmod form of navgpu_shortest_angular_distance. */
int navgpu_rotate_recovery_step(navgpu_fleet* fleet, uint32_t first, uint32_t count, const double* poses_xyth,
                                navgpu_rotate_recovery_state* state_inout, double* cmd_wz_out, int32_t* status_out);

/* replaces: CarrotPlanner::makePlan's search (carrot_planner/src/carrot_planner.cpp:116-169) for one plan per robot of
 * [first, first+count), on the costmaps this fleet holds.  starts_xyth, goals_xyth = count x {x, y, yaw}.  The candidates
 * start + scale * (goal - start), yaw normalize_angle(start_yaw + scale * normalize_angle(goal_yaw - start_yaw)), with scale
 * from 1.0 by repeated -= 0.01 until it is negative (:131-153), of all plans are evaluated in one k_footprint_cost launch.
 * targets_xyth_out = the first legal candidate in that order; found_out = the number of candidates tried up to and
 * including it (1: the goal itself), or 0 with the target set to the start when none is legal (:136-143).  A robot with
 * fewer than 3 footprint vertices finds nothing (CarrotPlanner::footprintCost, :76-79). */
int navgpu_carrot_plan(navgpu_fleet* fleet, uint32_t first, uint32_t count, const double* starts_xyth, const double* goals_xyth,
                       int32_t allow_unknown, double* targets_xyth_out, int32_t* found_out);

/* ------------------------------------------------------------------------------------------ */
/* VoxelLayer debug outputs: voxel clouds and clearing endpoints from the resident grid         */
/* ------------------------------------------------------------------------------------------ */
#define NAVGPU_VOXEL_UNKNOWN 1 /* voxel_grid::UNKNOWN */
#define NAVGPU_VOXEL_MARKED 2  /* voxel_grid::MARKED  */

/* replaces: the loops of costmap_2d_cloud's voxelCallback (costmap_2d/src/costmap_2d_cloud.cpp:85-122; float xyz, a
 * geometry_msgs::Point32 per voxel) and costmap_2d_markers' (costmap_2d/src/costmap_2d_markers.cpp:84-108; as_double = 1,
 * a geometry_msgs::Point per voxel) over the voxel_grid message, on the RESIDENT voxel grid (NAVGPU_GRID_VOXEL) of every
 * robot in [first, first+count).  Returned per robot: every voxel (x, y, z), z < z_voxels, whose VoxelGrid::getVoxel
 * (voxel_grid/include/voxel_grid/voxel_grid.h:183-206) equals `status` - bits z and z + 16 of the column both set: MARKED,
 * exactly one: UNKNOWN, neither: FREE, never returned - in the reference's loop order, y outer, then x, z inner.  The
 * coordinates are mapToWorld3D (costmap_2d_cloud.cpp:36-42), origin + (m + 0.5) * resolution in double, with the robot's
 * current origin and the fleet resolution for x / y and origin_z / z_resolution of navgpu_obstacle_configure for z;
 * as_double = 0 narrows them to float as the assignment to a Point32 does.
 * xyz = count x capacity x 3 floats or doubles, robot r's points from r * capacity * 3; counts[r] is always the true
 * number, points beyond `capacity` are not written, and nothing is written behind a robot's last point.  xyz = NULL with
 * capacity = 0 counts only.  The positions come from a prefix sum, not from atomics: two calls give identical bytes.
 * NAVGPU_ERR_INVALID for a fleet without NAVGPU_LAYER_VOXEL, a status other than the two above, a range outside the fleet
 * (or of more than 65535 robots), xyz = NULL with a capacity; NAVGPU_ERR_STATE while a staged rolling-window origin has not
 * been applied by an update yet (as navgpu_footprint_cost).  Ordered on the fleet's stream behind whatever was queued
 * before; returns when the results are in the caller's buffers. */
int navgpu_voxel_points(navgpu_fleet* fleet, uint32_t first, uint32_t count, int status, int as_double, uint32_t capacity, void* xyz,
                        uint32_t* counts);

/* replaces: the clearing_endpoints cloud of VoxelLayer::raytraceFreespace (costmap_2d/plugins/voxel_layer.cpp:286-381).
 * For every robot of the range, the clearing observations its last navgpu_costmap_stage staged, in staging order; for each,
 * its points in cloud order; for every point that passes worldToMap3DFloat at :353 the clipped ray end (float)wpx,
 * (float)wpy, (float)wpz of :297-372 - the same fp64 sequence k_obstacle walks its rays with.  An observation without
 * points, or whose sensor origin fails worldToMap3DFloat (:277-284), yields none; so does every observation while the layer
 * is disabled (:121-122).  counts[r] = the robot's total; obs_counts = count x max_observations entries, one per staged
 * observation of the robot in staging order (0 for marking-only ones and beyond the staged ones), so a caller can publish
 * one cloud per observation as the reference does.  xyz, capacity and the errors are those of navgpu_voxel_points.
 * Valid once navgpu_costmap_update or navgpu_obstacle_update_bounds has consumed the staging - the reference clips with the
 * origin AFTER updateOrigin (:119-120) - and until the next stage: NAVGPU_ERR_STATE otherwise. */
int navgpu_voxel_clearing_endpoints(navgpu_fleet* fleet, uint32_t first, uint32_t count, uint32_t capacity, float* xyz,
                                    uint32_t* obs_counts, uint32_t* counts);

/* ------------------------------------------------------------------------------------------ */
/* costmap_2d::ObservationBuffer on the device: clouds and laser scans, resident until purged   */
/* ------------------------------------------------------------------------------------------ */
/* What costmap_2d::ObservationBuffer (costmap_2d/src/observation_buffer.cpp:66-256) and the sensor callbacks of ObstacleLayer
 * (plugins/obstacle_layer.cpp:252-338, 466-496) do, with the tf LOOK-UP left to the caller as navgpu_static_set_transform leaves
 * it: sensor data goes up once, in the sensor's own frame, and stays on the device until the reference would purge it.  Per
 * (robot, source) the time-ordered list is host metadata, the points live in a ring of `slots` slots on the device.  Times are
 * int64 nanoseconds (ros::Time / ros::Duration are integers; the purge test is an exact comparison).
 *
 * Arithmetic (the library is built with -ffp-contract=off; nothing below is fused):
 *   cloud transform  pcl_ros::transformAsMatrix + pcl::transformPointCloud are not in the reference tree; RESTATED here, parity
 *                    unpinned (as for tf): the 12 doubles of `transform` are narrowed to float, then in fp32, left to right,
 *                      x' = ((m00*x + m01*y) + m02*z) + m03      y' = ((m10*x + m11*y) + m12*z) + m13      z' likewise
 *                    with m03, m13, m23 the origin (transform[9..11]).
 *   height filter    keep iff (double)z' <= max_obstacle_height && (double)z' >= min_obstacle_height (:169-170); NaN drops.
 *   scan             laser_geometry is not in the tree either: projectLaser RESTATED, parity unpinned
 *                    (transformLaserScanToPointCloud into the scan's own frame reduces to it, both look-ups being the identity).
 *                    With inf_is_valid a range that is not finite and > 0 first becomes range_max - 0.0001f in float
 *                    (obstacle_layer.cpp:281-289).  Beam i is kept iff r >= range_min && r < range_max (NaN, -inf, and +inf
 *                    without the flag drop out); its point is x = (float)((double)r * cos(a)), y = (float)((double)r * sin(a)),
 *                    z = 0 with a = (double)angle_min + (double)i * (double)angle_increment and the device's double sincos
 *                    (navgpu_device_sincos returns the same values); the cloud transform follows.  The per-beam time
 *                    interpolation of a scan taken while the sensor moves is not done.
 * Two stated departures from the reference: a list is bounded by `slots` (the reference's is unbounded) - an entry pushed out
 * is counted as `evicted`; and the capacity check of navgpu_obsbuf_stage uses the UNFILTERED sizes of the kept clouds, the
 * host never learning a filtered count on that path. */
typedef struct {                     /* one entry of observation_sources (obstacle_layer.cpp:96-140) */
  int64_t observation_keep_time_ns;  /* 0: keep only the newest (observation_buffer.cpp:217-221) */
  int64_t expected_update_rate_ns;   /* 0: always current (:240-241) */
  double min_obstacle_height, max_obstacle_height; /* the BUFFER's filter, :169-170 */
  double obstacle_range, raytrace_range;           /* copied into every observation, :151-152 */
  uint32_t flags;                    /* NAVGPU_OBS_MARKING | NAVGPU_OBS_CLEARING */
  int32_t inf_is_valid;              /* scans: laserScanValidInfCallback instead of laserScanCallback */
} navgpu_obs_source_params;

#define NAVGPU_OBSBUF_MAX_SOURCES 8
#define NAVGPU_OBSBUF_MAX_CLOUD_POINTS 65536
#define NAVGPU_CLOUD_XYZ 0           /* float xyz in the cloud's frame (pointCloud2Callback) */
#define NAVGPU_CLOUD_SCAN 1          /* float ranges (laserScanCallback / laserScanValidInfCallback) */
typedef struct {
  uint32_t instance, source, kind;
  uint32_t first, n;                 /* into points_xyz (points) or ranges (beams) of the call */
  uint32_t reserved;
  int64_t stamp_ns;                  /* cloud.header.stamp */
  double origin[3];                  /* tf_.transformPoint(global, (0,0,0) of sensor_frame / cloud frame), :142-148 */
  double transform[12];              /* global <- cloud frame: basis row-major, then origin (tf::Transform) */
  float angle_min, angle_increment, range_min, range_max; /* SCAN only */
} navgpu_cloud;

typedef struct {
  uint32_t kept;                     /* observations in the robot's lists */
  uint32_t points;                   /* their points after the height filter (read back from the device) */
  uint64_t evicted;                  /* entries pushed out of a full ring since configure */
  int32_t current;                   /* isCurrent of every source at the `now_ns` the last buffer / stage / reset call gave */
  int32_t reserved;
} navgpu_obsbuf_robot_status;

/* Any navgpu_obsbuf_* call but this one returns NAVGPU_ERR_STATE before a successful configure.
 * Allocates, per (robot, source), a ring of slots x max_cloud_points x 3 floats and slots counts; empties every list, zeroes
 * `evicted` and sets every last_updated to 0 (call navgpu_obsbuf_reset_last_updated as ObstacleLayer::activate does).
 * NAVGPU_ERR_INVALID unless 1 <= n_sources <= 8, 1 <= slots, 1 <= max_cloud_points <= 65536 and slots * n_sources <=
 * max_observations of the fleet.  All-or-nothing: a failed call leaves the previous configuration, and its lists, in force. */
int navgpu_obsbuf_configure(navgpu_fleet* fleet, const navgpu_obs_source_params* sources, uint32_t n_sources, uint32_t slots,
                            uint32_t max_cloud_points);
/* replaces: ObservationBuffer::bufferCloud (:129-195) behind pointCloud2Callback / laserScanCallback / laserScanValidInfCallback
 * (obstacle_layer.cpp:252-338) for each cloud of the call, in call order: push_front, origin and ranges, transform, height
 * filter in cloud order into a slot, last_updated = now_ns, purgeStaleObservations (:211-236: the newest only with a keep time
 * of 0, else everything from the first entry with last_updated - stamp > keep_time on).  A list longer than `slots` then loses
 * its oldest entry (counted as evicted).  NAVGPU_ERR_CAPACITY for a cloud with n > max_cloud_points; NAVGPU_ERR_INVALID for a
 * bad instance / source / kind, a range outside points_xyz / ranges, a non-finite transform or origin; a failing call buffers
 * nothing.  Asynchronous on the fleet's stream: one host-to-device copy of the call's points and ranges out of a pinned mirror
 * and one launch (k_obs_ingest); the host does not learn a filtered count here. */
int navgpu_obsbuf_buffer(navgpu_fleet* fleet, const navgpu_cloud* clouds, uint32_t n_clouds, const float* points_xyz, uint32_t n_points,
                         const float* ranges, uint32_t n_ranges, int64_t now_ns);
/* replaces: ObstacleLayer::getMarkingObservations + getClearingObservations (:466-496) + navgpu_costmap_stage for the range.
 * Per robot and source the list is purged as getObservations does (:198-209); one observation per kept entry is staged, sources
 * in configuration order, each newest first, with the source's flags (k_obstacle clears with every clearing observation before
 * it marks with any: one descriptor with both bits equals the reference's two passes).  current_out[r] (or NULL) = AND over
 * the sources of expected_update_rate == 0 || now_ns - last_updated <= expected_update_rate (:238-251).  Pose, transformed
 * footprint and rolling-window origin are staged exactly as navgpu_costmap_stage stages them, and everything around the call
 * (NAVGPU_ERR_STATE for a staged rolling-window shift not yet consumed, two cycles in flight, navgpu_voxel_clearing_endpoints
 * after the update) behaves as after it.  NAVGPU_ERR_CAPACITY, nothing staged, when the UNFILTERED sizes of a robot's kept
 * clouds sum to more than max_points. */
int navgpu_obsbuf_stage(navgpu_fleet* fleet, uint32_t first, uint32_t count, const double* robot_poses, int64_t now_ns, int32_t* current_out);
/* navgpu_obsbuf_stage for a robot list (the conventions of navgpu_costmap_stage_list; current_out is indexed by list position).
 * replaces: ObstacleLayer::getMarkingObservations + getClearingObservations (:466-496) over ObservationBuffer::getObservations
 * (observation_buffer.cpp:198-209) and isCurrent (:238-251), for the listed robots: the purge, last_updated and isCurrent rules are
 * the range form's; the descriptors travel in the packed upload and k_obs_gather runs once, on the list. */
int navgpu_obsbuf_stage_list(navgpu_fleet* fleet, uint32_t n_robots, const uint32_t* instances, const double* robot_poses, int64_t now_ns,
                             int32_t* current_out);
/* Synchronous read-back, for tests and debugging, of exactly what navgpu_obsbuf_stage would hand over for one robot: the
 * descriptors with the filtered n_points (first_point into points_xyz) and the global-frame points.  Changes no state (now_ns
 * is accepted for symmetry: the purge compares with last_updated).  Returns the number of observations, n_points_out the
 * points; NAVGPU_ERR_CAPACITY when either buffer is too small. */
int navgpu_obsbuf_observations(navgpu_fleet* fleet, uint32_t instance, int64_t now_ns, navgpu_observation* obs, uint32_t obs_capacity,
                               float* points_xyz, uint32_t point_capacity, uint32_t* n_points_out);
/* replaces: ObservationBuffer::setGlobalFrame (:66-109) with the looked-up transform M = new_global <- global, 12 doubles per
 * robot as above: every kept origin becomes M * origin in fp64 (tf::Transform::operator*: row . v + origin), every kept point
 * M * p by the cloud transform above, in place; nothing is filtered again (the reference does not). */
int navgpu_obsbuf_set_global_frame(navgpu_fleet* fleet, uint32_t first, uint32_t count, const double* transforms12);
/* replaces: ObservationBuffer::resetLastUpdated (:253-256) of every source, as ObstacleLayer::activate does */
int navgpu_obsbuf_reset_last_updated(navgpu_fleet* fleet, uint32_t first, uint32_t count, int64_t now_ns);
int navgpu_obsbuf_status(navgpu_fleet* fleet, uint32_t first, uint32_t count, navgpu_obsbuf_robot_status* out);

/* ------------------------------------------------------------------------------------------ */
/* measurement                                                                                */
/* ------------------------------------------------------------------------------------------ */
typedef enum {
  NAVGPU_K_OBSTACLE = 0, /* raytrace + mark + bounds                      */
  NAVGPU_K_MERGE = 1,    /* window reset + static/obstacle merge          */
  NAVGPU_K_INFLATE = 2,  /* inflation                                     */
  NAVGPU_K_BFS = 3,      /* MapGrid wavefronts                            */
  NAVGPU_K_SCORE = 4,    /* rollout + critics                             */
  NAVGPU_K_SELECT = 5,   /* argmin + result + oscillation update          */
  NAVGPU_K_FOOTPRINT = 6,/* batched footprint-cost queries                */
  NAVGPU_K_VOXEL_EXPORT = 7, /* voxel points / clearing endpoints: count, scan and emit launches */
  NAVGPU_K_OBS_INGEST = 8,   /* observation buffer: transform + filter + compaction of the clouds of a call */
  NAVGPU_K_CHECK_TRAJ = 9,  /* batched checkTrajectory: the probes of a robot list (navgpu_planner_check_trajectories) */
  NAVGPU_K_COUNT = 10
} navgpu_kernel_id;
/* HIP-event timing of the kernels on the fleet's stream.  While enabled every launch of the
 * listed kernels is bracketed by two hipEventRecord calls; read() synchronises and returns the
 * accumulated device time (ms) and launch count since the last reset. */
int navgpu_profile_enable(navgpu_fleet* fleet, int32_t enable);
/* restrict the bracketing to some kernels: bit k = navgpu_kernel_id k (default: all).  Every pair of events costs the
 * stream a few microseconds, so a throughput measurement selects the kernel it reports on. */
int navgpu_profile_select(navgpu_fleet* fleet, uint32_t kernel_mask);
int navgpu_profile_reset(navgpu_fleet* fleet);
int navgpu_profile_read(navgpu_fleet* fleet, int32_t kernel, double* total_ms, uint64_t* launches);
const char* navgpu_kernel_name(int32_t kernel);

/* The floating-point contract, checkable: sin / cos of `n` headings exactly as the scoring kernels evaluate them on `device`
 * (double `sincos`, the reference's `cos(theta)` / `sin(theta)` of simple_trajectory_generator.cpp:253-258 on the host's
 * libm).  Host pointers.  tests/ compare the result with the host's libm bit for bit and bound the difference. */
int navgpu_device_sincos(int32_t device, const double* theta, uint32_t n, double* sin_out, double* cos_out);

/* ------------------------------------------------------------------------------------------ */
/* navfn::NavFn - global-planner potential expansion and path extraction       */
/* ------------------------------------------------------------------------------------------ */
/* A batch of independent plans on maps of one size (one plan per robot of a fleet).  What is computed is exactly what
 * navfn::NavFn computes - potentials, priority-buffer order, the early stop at the start cell, the interpolated path -
 * bit for bit (the expansion is an order-dependent sequential process: one GPU lane walks each plan, the batch is the
 * parallel dimension).  Coordinates are cells, origin upper left, as in the reference (navfn.h:108-112). */
typedef struct navgpu_navfn navgpu_navfn;
typedef struct {
  int32_t found;          /* calcNavFnDijkstra / calcNavFnAstar return value (navfn.cpp:293-345)           */
  int32_t path_length;    /* NavFn::getPathLen(), 0 when no path was found                                 */
  int32_t cycles;         /* propagation cycles used                                                       */
  float start_potential;  /* potarr[start] (NavFn::getLastPathCost after calcNavFnAstar)                   */
} navgpu_navfn_result;
/* replaces: NavFn::NavFn / setNavArr (navfn.cpp:110-215) for n_plans plans */
int navgpu_navfn_create(uint32_t nx, uint32_t ny, uint32_t n_plans, int32_t device, navgpu_navfn** out);
int navgpu_navfn_destroy(navgpu_navfn* nav);
/* replaces: NavFn::setCostmap(cmap, isROS, allow_unknown) (navfn.cpp:222-283).  cmap = count x ny x nx bytes (or ONE map shared
 * by all plans when shared != 0).  cost_mode 1: isROS = true (costmap_2d values), 2: isROS = false (a plain PGM, 7-cell
 * borders stay obstacles), 0: the bytes are costarr itself (navfn/test/path_calc_test.cpp:52) */
int navgpu_navfn_set_costmap(navgpu_navfn* nav, uint32_t first, uint32_t count, const uint8_t* cmap, int32_t shared, int32_t cost_mode,
                             int32_t allow_unknown);
/* the same from the master grids of a fleet on the same GPU (NavfnROS::makePlan hands costmap_->getCharMap() over, navfn_ros.cpp:265-268):
 * plan first + k takes the master grid of fleet instance fleet_first + k; nothing crosses PCIe */
int navgpu_navfn_set_costmap_from_fleet(navgpu_navfn* nav, uint32_t first, uint32_t count, navgpu_fleet* fleet, uint32_t fleet_first,
                                        int32_t allow_unknown);
/* replaces: the same hand-over (navfn_ros.cpp:265-268; planner_core.cpp:290 for cost_mode 0) where a run of plans works on ONE
 * robot's costmap - the candidate goals of navgpu_move_base_plan_service: every plan of [first, first+count) takes the master grid
 * of fleet instance `instance`, through cost_mode as in navgpu_navfn_set_costmap */
int navgpu_navfn_set_costmap_from_fleet_instance(navgpu_navfn* nav, uint32_t first, uint32_t count, navgpu_fleet* fleet, uint32_t instance,
                                                 int32_t cost_mode, int32_t allow_unknown);
/* replaces: NavFn::setGoal / setStart + calcNavFnDijkstra(at_start) | calcNavFnAstar() (navfn.cpp:145-171, 293-345).
 * goals_xy, starts_xy = count x {x, y} cells.  (NavfnROS passes the robot as "goal" and the goal as "start",
 * navfn_ros.cpp:270-281: the potential is grown from the robot.) */
int navgpu_navfn_plan(navgpu_navfn* nav, uint32_t first, uint32_t count, const int32_t* goals_xy, const int32_t* starts_xy, int32_t astar,
                      int32_t at_start, navgpu_navfn_result* results);
/* The same call as a device algorithm (no counterpart in the reference): NavFn::updateCell's update rule (navfn.cpp:466-535,
 * same float / double arithmetic) relaxed to its fixed point by 32 x 32 tiles in LDS, round by round, instead of walked
 * through the three priority buffers on one lane; at_start stops once the start cell and everything below its potential
 * is final (the counterpart of :692-694).  The potentials are those the reference's process converges to where it is
 * allowed to finish: <= the reference's everywhere (its 10 000-entry buffers drop cells, its push tests skip updates, its
 * early stop leaves the last block half done), equal along most of the path; calcPath (the same code) then gives a path
 * within a fraction of a cell of the reference's (tests/test_navfn.py: Hausdorff distance <= 1 cell on the reference's
 * willow_costmap searches).  Results do not depend on scheduling (rounds are Jacobi across tiles, tiles are swept
 * red / black).  results[k].cycles = rounds run.  Dijkstra only.  The bit-exact mode stays navgpu_navfn_plan. */
int navgpu_navfn_plan_wavefront(navgpu_navfn* nav, uint32_t first, uint32_t count, const int32_t* goals_xy, const int32_t* starts_xy,
                                int32_t at_start, navgpu_navfn_result* results);
/* replaces: NavFn::getPathX / getPathY / getPathLen: xy = up to capacity_points x {x, y}; returns the path length */
int navgpu_navfn_path(navgpu_navfn* nav, uint32_t plan, float* xy, uint32_t capacity_points);
/* NavFn::potarr of one plan (ny x nx floats, POT_HIGH = 1e10 where unassigned) */
int navgpu_navfn_potential(navgpu_navfn* nav, uint32_t plan, float* potarr);
/* NavFn::costarr of one plan (ny x nx bytes): what the last navgpu_navfn_set_costmap / _from_fleet wrote for it.  A plan call
 * afterwards outlines the array's border with COST_OBS, as NavFn::setupNavFn does (navfn.cpp:412-425). */
int navgpu_navfn_costarr(navgpu_navfn* nav, uint32_t plan, uint8_t* costarr);

/* global_planner::GlobalPlanner's expansion and traceback on the same arrays (the other half of SURVEY 8 f-4).
 * Parameters as planner_core.cpp:105-152 reads them and GlobalPlanner.cfg sets them. */
typedef struct {
  int32_t use_dijkstra;       /* 1: DijkstraExpansion (dijkstra.cpp), 0: AStarExpansion (astar.cpp)                          */
  int32_t use_quadratic;      /* 1: QuadraticCalculator, 0: PotentialCalculator                                              */
  int32_t use_grid_path;      /* 1: GridPath, 0: GradientPath                                                                */
  int32_t old_navfn_behavior; /* 1: integer start / goal, no precise start, no clearEndpoint (planner_core.cpp:108-127,299)  */
  int32_t allow_unknown;      /* Expander::setHasUnknown                                                                     */
  int32_t lethal_cost, neutral_cost; /* GlobalPlanner.cfg: 253, 50                                                           */
  float cost_factor;          /* GlobalPlanner.cfg: 3.0                                                                      */
  int32_t outline_map;        /* 1: GlobalPlanner::outlineMap(costs, nx, ny, LETHAL_OBSTACLE) first, as makePlan does (:296).
                               * With 0, or with lethal_cost 255 under A*, border cells can be expanded; the reference then
                               * reads potential[] / costs[] one row outside its arrays.  Here such neighbours read as
                               * unreached lethal cells (never outside device memory); results on maps whose expansion
                               * stays off the border are unchanged                                                          */
  int32_t reserved;
} navgpu_global_planner_params;
/* replaces: the body of GlobalPlanner::makePlan between worldToMap and the plan assembly (planner_core.cpp:250-311):
 * outlineMap, planner_->calculatePotentials(costs, start, goal, nx * ny * 2, potential), clearEndpoint, path_maker_->getPath.
 * The cost bytes are those of navgpu_navfn_set_costmap with cost_mode 0 (the costmap itself: getCost translates on the fly).
 * starts_xy / goals_xy = count x {x, y} MAP coordinates as makePlan computes them (the cell index, or (w - origin) / resolution
 * - 0.5 without old_navfn_behavior); goal_cells_xy = count x {goal_x_i, goal_y_i}.  navgpu_navfn_path then returns the
 * traceback's own point list (goal first; getPlanFromPotential reverses it), navgpu_navfn_potential the potential array.
 * Limits: starts closer than 2 cells and goals closer than 1 cell to the map border are rejected (the reference reads
 * outside its arrays there); a traceback longer than max(nx * ny / 2, 4 nx) + 4 points - the reference allows 4 nx ny -
 * reports found = 0. */
int navgpu_global_planner_plan(navgpu_navfn* nav, uint32_t first, uint32_t count, const navgpu_global_planner_params* params,
                               const double* starts_xy, const double* goals_xy, const int32_t* goal_cells_xy, navgpu_navfn_result* results);
/* The same call with DijkstraExpansion run as a device algorithm (see navgpu_navfn_plan_wavefront: the update rule of
 * dijkstra.cpp:170-229 - getCost, PotentialCalculator or QuadraticCalculator - relaxed to its fixed point by LDS tiles from the
 * start cell(s), stopped once the goal cell and everything below its potential is final); clearEndpoint and the traceback are
 * the same code as in navgpu_global_planner_plan.  use_dijkstra must be 1.  results[k].cycles = rounds run. */
int navgpu_global_planner_plan_wavefront(navgpu_navfn* nav, uint32_t first, uint32_t count, const navgpu_global_planner_params* params,
                                         const double* starts_xy, const double* goals_xy, const int32_t* goal_cells_xy, navgpu_navfn_result* results);

/* GlobalPlanner::makePlan end to end, world coordinates in and world poses out, for a batch of plans. */
#define NAVGPU_ORIENT_NONE 0      /* GlobalPlanner.cfg orientation_mode, orientation_filter.h:43 */
#define NAVGPU_ORIENT_FORWARD 1
#define NAVGPU_ORIENT_INTERPOLATE 2
#define NAVGPU_ORIENT_FORWARD_THEN_INTERPOLATE 3

#define NAVGPU_MAKE_PLAN_OK 0
#define NAVGPU_MAKE_PLAN_START_OFF_MAP 1  /* Costmap2D::worldToMap fails, planner_core.cpp:256-260 */
#define NAVGPU_MAKE_PLAN_GOAL_OFF_MAP 2   /* :271-275 */
#define NAVGPU_MAKE_PLAN_NO_PLAN 3        /* found_legal false, or "NO PATH!": the reference returns an empty plan */
#define NAVGPU_MAKE_PLAN_BORDER 4         /* the library's own limit: start < 2 cells, goal < 1 cell from the border */

typedef struct { double x, y, yaw; } navgpu_global_pose;
typedef struct {
  int32_t orientation_mode;  /* NAVGPU_ORIENT_*                                                                  */
  int32_t wavefront;         /* 1: the expansion of navgpu_global_planner_plan_wavefront (use_dijkstra must be 1) */
} navgpu_make_plan_options;
typedef struct {
  int32_t status;            /* NAVGPU_MAKE_PLAN_*                                                                */
  int32_t n_poses;           /* path_length + 1 (+ 2 with old_navfn_behavior); 0 unless status is OK              */
  int32_t found, cycles;     /* as navgpu_navfn_result; 0 for a plan that was not attempted                       */
  int32_t start_cell[2], goal_cell[2]; /* Costmap2D::worldToMap's cells (what it succeeded for)                   */
  float start_potential;
  int32_t reserved;
} navgpu_make_plan_result;
/* replaces: GlobalPlanner::makePlan (planner_core.cpp:222-327) without its frame checks and publishers, for the plans
 * [first, first+count): Costmap2D::worldToMap of start and goal (costmap_2d.cpp:208-220), GlobalPlanner::worldToMap (:201-215;
 * its return value is ignored, as makePlan ignores it), clearRobotCell (:176-185, 283-286), the core of
 * navgpu_global_planner_plan (or _plan_wavefront with options->wavefront), getPlanFromPotential (:351-395) with goal_copy
 * (:306-312), and OrientationFilter::processPath (orientation_filter.cpp:53-111) on yaws.
 * frames = count x {origin_x, origin_y, resolution} (the costmap of each plan); starts_xyyaw / goals_xyyaw = count x
 * {x, y, yaw} in the world.  The cost bytes are those set with cost_mode 0.  clearRobotCell writes FREE_SPACE (0) to the start
 * cell of the plan's own cost array on the device; it stays there until the next navgpu_navfn_set_costmap*, as the reference's
 * write stays in its costmap.
 * A plan whose status is not OK is not attempted (START_OFF_MAP, GOAL_OFF_MAP, BORDER) or came back empty (NO_PLAN); it does
 * not disturb the others and is no error of the call.  tolerance, planner_window_x/y and default_tolerance have no effect in
 * the reference and no counterpart here.
 * The assembled plan: the traceback's points in reverse order, each origin + ((double)point + convert_offset) * resolution
 * with yaw 0; the goal pose with old_navfn_behavior; the goal pose (goal_copy).  Then, with n = n_poses:
 *   FORWARD      yaw[i] = atan2(y[i+1] - y[i], x[i+1] - x[i]) for i < n - 1
 *   INTERPOLATE  yaw[0] = the start's yaw, then interpolate(0, n - 1)
 *   FORWARD_THEN_INTERPOLATE  FORWARD; i = n - 3, last = yaw[i]; while i > 0 and |shortest_angular_distance(yaw[i-1], last)|
 *                <= 0.35: --i (last is never updated, :72-81); yaw[0] = the start's yaw; interpolate(i, n - 1).  For n < 3 the
 *                reference reads before its array; the library takes i = 0.
 *   interpolate(a, b): increment = shortest_angular_distance(yaw[a], yaw[b]) / (b - a); yaw[i] = yaw[a] + increment * i for
 *                a <= i <= b - the absolute i, as written (:107-110) - not normalised.
 * shortest_angular_distance is navgpu_shortest_angular_distance (the fmod form).  The reference carries the yaws through
 * quaternions (tf::createQuaternionMsgFromYaw / tf::getYaw, outside the reference tree); the library keeps yaws.
 * Returns NAVGPU_ERR_INVALID for a bad range, a resolution that is not positive, an orientation_mode outside 0..3, the
 * parameter limits of navgpu_global_planner_plan, or wavefront without use_dijkstra. */
int navgpu_global_planner_make_plan(navgpu_navfn* nav, uint32_t first, uint32_t count, const navgpu_global_planner_params* params,
                                    const navgpu_make_plan_options* options, const double* frames, const double* starts_xyyaw,
                                    const double* goals_xyyaw, navgpu_make_plan_result* results);
/* replaces: the plan vector GlobalPlanner::makePlan fills (planner_core.cpp:306-321), for the plans [first, first+count) as
 * the last navgpu_global_planner_make_plan left them, concatenated in plan order: offsets[k] = first pose of plan first + k,
 * offsets[count] = the total.  Offsets are always true; poses at or beyond capacity are not written; poses = NULL with
 * capacity = 0 counts only (navgpu_voxel_points' conventions).  One device pass and one copy for the whole range; two calls
 * give identical bytes.  NAVGPU_ERR_STATE if, for a plan of the range, make_plan is not the last call that set its costs or
 * planned on it. */
int navgpu_global_planner_plans(navgpu_navfn* nav, uint32_t first, uint32_t count, uint32_t capacity, navgpu_global_pose* poses,
                                uint32_t* offsets);
/* replaces: GlobalPlanner::publishPotential's data (planner_core.cpp:417-434) for the plans [first, first+count): grids = count
 * x ny x nx bytes, maxima (may be NULL) = count floats.  max over the cells with potential < POT_HIGH; a cell is -1 where the
 * potential is >= POT_HIGH, else (int8)(potential * publish_scale / max) in float arithmetic as written.  Where max == 0 the
 * reference divides by zero; the library writes 0.  Reads the array that holds the plan's last result (as
 * navgpu_navfn_potential).  The message's origin (:411-413) is the caller's. */
int navgpu_global_planner_potential_grid(navgpu_navfn* nav, uint32_t first, uint32_t count, int32_t publish_scale, int8_t* grids,
                                         float* maxima);

/* navfn::NavfnROS (navfn/src/navfn_ros.cpp) round the same handle: makePlan end to end and the potential queries, for a batch of
 * plans.  The cost bytes are those of navgpu_navfn_set_costmap with cost_mode 1 or of navgpu_navfn_set_costmap_from_fleet:
 * makePlan hands getCharMap() to setCostmap(.., true, allow_unknown) (:263-264).  frames = count x {origin_x, origin_y,
 * resolution}, as in navgpu_global_planner_make_plan; every call returns NAVGPU_ERR_INVALID for a bad range, a NULL argument
 * or a resolution that is not positive.  The NAVGPU_MAKE_PLAN_* statuses are reused; BORDER does not occur. */
#define NAVGPU_NAVFN_ROS_MAX_WINDOW 4096 /* candidates per axis of a tolerance window */
typedef struct {
  double tolerance_weight_dist_from_goal; /* the window's cost = dist * this + potential * the next (:316-317) */
  double tolerance_weight_path_length;
  int32_t wavefront;                      /* 1: the expansion of navgpu_navfn_plan_wavefront                   */
  int32_t reserved;
} navgpu_navfn_ros_params;
typedef struct {
  int32_t status;            /* NAVGPU_MAKE_PLAN_*                                                                       */
  int32_t n_poses;           /* poses of the plan; 0 unless status is OK                                                 */
  int32_t found, cycles;     /* calcNavFnDijkstra's return value (which makePlan ignores) and cycles; 0 if not attempted */
  int32_t start_cell[2];     /* the robot's cell: NavFn's goal                                                           */
  int32_t goal_cell[2];      /* the goal's (or the point's) cell; (0, 0) where worldToMap failed                         */
  int32_t best_cell[2];      /* the cell of the window's best candidate, (-1, -1) without one                            */
  int32_t candidates;        /* window candidates with potential < POT_HIGH                                              */
  float start_potential;     /* potarr[NavFn's start] after the expansion                                                */
  double best_x, best_y;     /* best_pose's position (:321)                                                              */
  double best_cost;          /* its cost                                                                                 */
} navgpu_navfn_ros_result;
typedef struct { float x, y, z, pot_value; } navgpu_navfn_ros_cloud_point; /* PotarrPoint (navfn/potarr_point.h) */

/* replaces: NavfnROS::makePlan(start, goal, tolerance, plan) (navfn_ros.cpp:218-374) without its frame checks and publishers,
 * for the plans [first, first+count).  starts_xyyaw / goals_xyyaw = count x {x, y, yaw} in the world, tolerances = count doubles
 * (the overload without a tolerance, :213-216, is the caller passing default_tolerance).  As written there:
 *   worldToMap(start) fails -> START_OFF_MAP; worldToMap(goal) fails -> GOAL_OFF_MAP if tolerance <= 0, else the goal's cell is
 *   (0, 0) (:282-289); NavFn's goal is the robot's cell and NavFn's start the goal's; calcNavFnDijkstra(true) through
 *   navgpu_navfn_plan's bit-exact kernel (or navgpu_navfn_plan_wavefront's rounds with params->wavefront), its return value
 *   ignored.  clearRobotCell is NOT called: this makePlan never calls it.
 *   The tolerance window (:301-327): p.y = goal.y - tolerance, += resolution while <= goal.y + tolerance, inside it p.x
 *   likewise - sequential fp64 sums, built on the host; for each candidate the potential of its cell (DBL_MAX off the map), a
 *   candidate if < POT_HIGH, cost = sqrt(dx * dx + dy * dy) * tolerance_weight_dist_from_goal + potential *
 *   tolerance_weight_path_length in fp64; the first candidate in scan order (y outer, x inner) of the lowest cost below DBL_MAX
 *   is best_pose.  tolerance == 0 is one candidate; tolerance < 0 or NaN none (NO_PLAN).  One workgroup per plan, reduced
 *   without atomics: a pure function of the inputs.
 *   With a best_pose, getPlanFromPotential(best_pose) (:400-461): calcPath(4 nx) from its cell to the robot's over the same
 *   potential; an empty path is NO_PLAN ("Failed to get a plan from potential when a legal potential was found").  The plan:
 *   the path's points in reverse order, each origin + (double)point * resolution with yaw 0, then best_pose with the goal's
 *   yaw (:333-335): n_poses = path length + 1.
 * Limit: more than NAVGPU_NAVFN_ROS_MAX_WINDOW candidates on an axis of a window (tolerance > ~2048 resolution, or a sum that no
 * longer moves) is NAVGPU_ERR_INVALID for the call; nothing has run then.  From the cells (0, 1) and (0, ny - 1) the
 * reference's calcPath reads one element outside potarr; the library ends that walk as the reference does when those
 * elements hold ordinary values (no path); a walk that only arrives on one of those two cells reads them, as in navgpu_navfn_plan.
 * Departure: where calcPath fails after walking some points (out of steps, zero gradient, high potential) the reference's
 * getPlanFromPotential reads getPathLen(), the points walked so far, and returns them as a plan; the library reports NO_PLAN and
 * no poses, here and in navgpu_navfn_ros_plan_from_potential.
 * Parity is bit for bit against the reference built with C's <math.h>, where NavFn's hypot on floats is hypot(double, double) (as
 * navgpu_navfn_plan's walk has always restated it); with libstdc++'s math.h from GCC 6 on the same source calls hypotf and a
 * few path points differ in the last bit.
 * A plan whose status is not OK does not fail the call or disturb the others.  navgpu_navfn_potential then returns the
 * potential, navgpu_navfn_path the second path (nothing for a plan whose status is not OK). */
int navgpu_navfn_ros_make_plan(navgpu_navfn* nav, uint32_t first, uint32_t count, const navgpu_navfn_ros_params* params, const double* frames,
                               const double* starts_xyyaw, const double* goals_xyyaw, const double* tolerances,
                               navgpu_navfn_ros_result* results);
/* replaces: the plan vector NavfnROS::makePlan / getPlanFromPotential fills (:331-336, 440-456), for the plans [first, first+count)
 * as the last navgpu_navfn_ros_make_plan or navgpu_navfn_ros_plan_from_potential left them.  Conventions are
 * navgpu_global_planner_plans': offsets always true, poses beyond capacity not written, NULL with capacity 0 counts only, one
 * device pass and one copy.  NAVGPU_ERR_STATE if, for a plan of the range, neither of the two is the last call that set its
 * costs or planned on it (navgpu_global_planner_make_plan included: the two families do not read each other's plans). */
int navgpu_navfn_ros_plans(navgpu_navfn* nav, uint32_t first, uint32_t count, uint32_t capacity, navgpu_global_pose* poses, uint32_t* offsets);
/* replaces: NavfnROS::getPlanFromPotential(goal, plan) (:400-461) on the potential each plan holds: worldToMap(goal) fails ->
 * GOAL_OFF_MAP; setStart(goal's cell); calcPath(4 nx) to NavFn's goal, which is that of the last navgpu_navfn_ros_make_plan /
 * _compute_potential on the plan ((0, 0) before any; results[k].start_cell reports it).  The plan is the reversed path, no goal
 * appended: n_poses = path length, 0 -> NO_PLAN.  results[k].found = the walk's. */
int navgpu_navfn_ros_plan_from_potential(navgpu_navfn* nav, uint32_t first, uint32_t count, const double* frames, const double* goals_xyyaw,
                                         navgpu_navfn_ros_result* results);
/* replaces: NavfnROS::computePotential(world_point) (:171-197): points_xy = count x {x, y}; worldToMap fails -> status
 * GOAL_OFF_MAP (the reference returns false) and nothing runs for that plan; else NavFn's goal = the point's cell, start =
 * (0, 0), calcNavFnDijkstra() without the early stop; results[k].found is its return value.  params: only wavefront is read. */
int navgpu_navfn_ros_compute_potential(navgpu_navfn* nav, uint32_t first, uint32_t count, const navgpu_navfn_ros_params* params,
                                       const double* frames, const double* points_xy, navgpu_navfn_ros_result* results);
/* replaces: NavfnROS::getPointPotential (:157-169), batched: plan first + k has query_counts[k] points, packed in plan order in
 * points_xy; potentials[q] = (double)potarr[cell], DBL_MAX where worldToMap fails.  One lane per query on the resident array. */
int navgpu_navfn_ros_point_potential(navgpu_navfn* nav, uint32_t first, uint32_t count, const double* frames, const uint32_t* query_counts,
                                     const double* points_xy, double* potentials);
/* replaces: NavfnROS::validPointPotential(world_point, tolerance) (:130-155), batched as above with a tolerance per point:
 * flags[q] = 1 if any candidate of the window (sequences as in make_plan) has potential < POT_HIGH.  The same limit of
 * NAVGPU_NAVFN_ROS_MAX_WINDOW candidates per axis. */
int navgpu_navfn_ros_valid_point_potential(navgpu_navfn* nav, uint32_t first, uint32_t count, const double* frames,
                                           const uint32_t* query_counts, const double* points_xy, const double* tolerances, int32_t* flags);
/* replaces: the `potential` topic's cloud (:342-368) for the plans [first, first+count): the cells with (double)potarr[i] < 10e7
 * in row-major order, x = (float)(origin_x + (double)(i % nx) * resolution), y likewise, z = potarr[i] / potarr[start] * 20 in
 * float arithmetic, pot_value = potarr[i].  start is NavFn's start cell as the last navgpu_navfn_ros_* call on the plan left it:
 * the best cell after a make_plan that found one, the goal's cell (or (0, 0)) after one that did not, (0, 0) after
 * compute_potential, the goal's cell after plan_from_potential; (0, 0) before any.  A zero or huge divisor gives what IEEE float
 * division gives; nothing is patched.  Plans are concatenated: offsets[k] = first point of plan first + k, offsets[count] = the
 * total, always true; points at or beyond capacity are not written; points = NULL with capacity 0 counts only.  The positions
 * come from a prefix sum, not from atomics: two calls give identical bytes.  count <= 65535 and count * nx * ny < 2^32. */
int navgpu_navfn_ros_potential_cloud(navgpu_navfn* nav, uint32_t first, uint32_t count, const double* frames, uint32_t capacity,
                                     navgpu_navfn_ros_cloud_point* points, uint32_t* offsets);

/* ------------------------------------------------------------------------------------------ */
/* move_base's planner-side executive for a fleet: polygon writes, clearing windows, the plan   */
/* handover with its persistence policy (move_base/src/move_base.cpp)                           */
/* ------------------------------------------------------------------------------------------ */
#define NAVGPU_MAX_POLYGON 256 /* vertices of one polygon of navgpu_costmap_set_polygon_cost */
/* replaces: Costmap2D::setConvexPolygonCost(polygon, cost_value) (costmap_2d.cpp:315-428: worldToMap of every vertex,
 * polygonOutlineCells' raytraceLine walk, convexFillCells' column fill) as a public operation, for robots [first, first+count) at
 * once: polygon k is polys_xy[offsets[k] .. offsets[k+1]) as world {x, y} pairs, written with `value` (any byte) into `grid` of
 * robot first + k.  grid is NAVGPU_GRID_MASTER (what MoveBase::clearCostmapWindows writes, move_base.cpp:304, 329) or
 * NAVGPU_GRID_OBSTACLE (what MoveSlowAndClear writes into its "obstacles" layers, move_slow_and_clear.cpp:109-127); anything else
 * is NAVGPU_ERR_INVALID, an obstacle grid the fleet does not have NAVGPU_ERR_STATE.
 * As in the reference: a vertex whose worldToMap fails gives ok_out[k] = 0 and nothing is written for that robot (the other
 * robots are unaffected; no error of the call); fewer than 3 vertices give ok_out[k] = 1 and nothing written; else per column
 * every cell from the lowest to the highest outline cell is written - which is what the bubble sort and pairwise walk of
 * convexFillCells amount to, for polygons that are not convex too (tests/test_gpu_polygon_cost.py holds it to the compiled
 * rule).  A polygon may have up to NAVGPU_MAX_POLYGON vertices (NAVGPU_ERR_CAPACITY above) and span any number of columns.
 * offsets must not decrease (NAVGPU_ERR_INVALID); ok_out may be NULL.  NAVGPU_ERR_STATE while a staged rolling-window origin has
 * not been applied by an update yet (the polygons are in world coordinates).  A call that fails changes nothing.  The layer's
 * bounds are not touched: the reference's callers do not touch them either (MoveSlowAndClear's write reaches the master grid
 * with the next update whose bounds cover it). */
int navgpu_costmap_set_polygon_cost(navgpu_fleet* fleet, int grid, uint32_t first, uint32_t count, const double* polys_xy,
                                    const uint32_t* offsets, uint8_t value, int32_t* ok_out);
/* replaces: one half of MoveBase::clearCostmapWindows(size_x, size_y) (move_base.cpp:277-330) - the reference clears the planner's
 * and the controller's costmap; here the caller names the fleet that holds each - for robots [first, first+count): poses_xy =
 * count x {x, y} (getRobotPose's origin), the polygon (x - size_x / 2, y - size_y / 2), (x + size_x / 2, y - size_y / 2),
 * (x + size_x / 2, y + size_y / 2), (x - size_x / 2, y + size_y / 2) in that order and those expressions, FREE_SPACE on the master
 * grid through navgpu_costmap_set_polygon_cost.  A window with a corner off the map clears nothing, as in the reference (which
 * ignores setConvexPolygonCost's return value); ok_out (may be NULL) reports it. */
int navgpu_move_base_clear_costmap_windows(navgpu_fleet* fleet, uint32_t first, uint32_t count, const double* poses_xy, double size_x,
                                           double size_y, int32_t* ok_out);

/* MoveBase::persistence_end_ per robot, held as the reference holds it: a time in ns whose two special values are times too */
#define NAVGPU_PERSISTENCE_INITIAL 0LL           /* PERSISTENCE_INITIAL = ros::Time(0, 0) (move_base.cpp:58)  */
#define NAVGPU_PERSISTENCE_NEWPLAN 1000000000LL  /* PERSISTENCE_NEWPLAN = ros::Time(1, 0) (:59)               */
typedef enum {
  NAVGPU_HANDOVER_NONE = 0,     /* the plan was not made (n_poses 0): new_global_plan_ is false, the robot and its state untouched */
  NAVGPU_HANDOVER_ADOPT = 1,    /* preferPrevPlan returned false: the new plan is the controller's plan                           */
  NAVGPU_HANDOVER_KEEP = 2,     /* it returned true: the controller keeps its plan, the caller replans (state_ = PLANNING)         */
  NAVGPU_HANDOVER_TOO_LONG = 3  /* the plan is longer than max_global_plan: the robot and its state untouched                      */
} navgpu_handover_decision;
typedef struct {
  int32_t decision;            /* navgpu_handover_decision                                                           */
  int32_t closest_index;       /* findClosestPlanIndex: an index of the controller plan as it was handed over        */
  int32_t prev_len;            /* prev_plan_len = controller_plan_->size() - closest_i                               */
  int32_t new_len;             /* latest_plan_->size()                                                               */
  int32_t dropped;             /* leading poses of the controller plan that are no longer stored (a store resize)    */
  int32_t reserved;
  int64_t persistence_end_ns;  /* the robot's state after the call                                                   */
} navgpu_handover_record;
/* replaces: executeCycle's `if(new_global_plan_ && !preferPrevPlan(current_position))` handing controller_plan_ to tc_->setPlan
 * (move_base.cpp:873-888) with MoveBase::preferPrevPlan and findClosestPlanIndex (:784-836), for robots [fleet_first,
 * fleet_first+count) and plans [nav_first, nav_first+count) of a NavFn handle.  The arguments of navgpu_local_planner_adopt_plans,
 * and: positions_xy = count x {x, y}, the robots' positions in their plans' frame; now_ns (ros::Time::now()); persistence_timeout_ns
 * (plan_persistence_timeout_, 10 s by default, :57); out = one record per robot (may be NULL).
 * Per robot whose plan was made and fits the store, on the device (k_plan_prefer, a workgroup per robot):
 *   closest_i  the first index with the strictly smallest hypot(pos.x - p.x, pos.y - p.y) below 1e9 over indices 0, 4, 8, ... of
 *              the controller plan AS IT WAS HANDED OVER - move_base's controller_plan_ is never pruned, and the store keeps the
 *              poses prunePlan erased in place; 0 when none is below 1e9 (NaN included), for an empty plan and for a robot without
 *              a resident plan (whose controller plan counts as empty).  hypot is restated (within 1 ulp of libm's): the index is
 *              libm's unless two sampled distances are closer than that.
 *   prev_len = original length - closest_i; prefer_prev = prev_len + 320 < new_len.
 *   If prefer_prev and the state is not INITIAL: a state of NEWPLAN becomes now + timeout; then now < state is KEEP.
 *   In every other case the state becomes NEWPLAN and the decision is ADOPT.
 * ADOPT is navgpu_local_planner_adopt_plans for that robot (slot written by the emit kernel, latch cleared, oscillation flags
 * reset); the emit kernel is predicated per robot on the decision, which has not left the device by then.  KEEP changes nothing
 * of the robot but its persistence state.  One record per robot is read back afterwards; no plan pose crosses the bus.
 * Departure: navgpu_local_planner_reserve_plans' resize carries only the live part of a plan over.  `dropped` counts the leading
 * poses lost that way; the search then visits the original indices >= dropped that are multiples of 4 (prev_len still counts
 * from the original length).
 * Returns as navgpu_local_planner_adopt_plans: NAVGPU_ERR_CAPACITY after handling the others when a plan is too long (its
 * record says TOO_LONG); NAVGPU_ERR_INVALID also for a NULL positions_xy or a negative timeout.  A call that fails with
 * NAVGPU_ERR_INVALID or NAVGPU_ERR_STATE has changed nothing.  NAVGPU_ERR_HIP (a launch or copy failed) may come after the device
 * has updated persistence states and written slots whose host bookkeeping was not done: hand those robots their plans again
 * (navgpu_local_planner_set_plans) and set their states before going on, as after any failed device call. */
int navgpu_move_base_handover_plans(navgpu_fleet* fleet, uint32_t fleet_first, navgpu_navfn* nav, uint32_t nav_first, uint32_t count,
                                    int32_t family, const double* plan_to_global, const double* positions_xy, int64_t now_ns,
                                    int64_t persistence_timeout_ns, navgpu_handover_record* out);
/* replaces: `persistence_end_ = PERSISTENCE_INITIAL` on a new goal (move_base.cpp:664, 707) for robots [first, first+count) */
int navgpu_move_base_reset_persistence(navgpu_fleet* fleet, uint32_t first, uint32_t count);
/* replaces: nothing in the reference, which keeps persistence_end_ private: the robots' states for tests and checkpoints,
 * count x int64 ns.  NAVGPU_ERR_STATE (all three calls) without a store (navgpu_local_planner_reserve_plans). */
int navgpu_move_base_get_persistence(navgpu_fleet* fleet, uint32_t first, uint32_t count, int64_t* persistence_end_ns);
int navgpu_move_base_set_persistence(navgpu_fleet* fleet, uint32_t first, uint32_t count, const int64_t* persistence_end_ns);

/* MoveBase::planService's search for a feasible goal (move_base.cpp:340-426) on a NavFn handle: every candidate goal of a request
 * is a plan of one batch. */
#define NAVGPU_PLAN_SERVICE_MAX_CANDIDATES 1024 /* candidates of one request, the exact goal included */
typedef struct {
  double start[3];           /* the start pose {x, y, yaw}: req.start, or the robot's pose (:355-360)                        */
  double goal[3];            /* req.goal                                                                                      */
  double frame[3];           /* {origin_x, origin_y, resolution} of the planner's costmap                                     */
  double tolerance;          /* req.tolerance                                                                                 */
  double default_tolerance;  /* navfn_ros family: what makePlan(start, goal, plan) hands on (navfn_ros.cpp:213-216); else unread */
} navgpu_plan_service_request;
typedef struct {
  int32_t winner;        /* index of the first candidate, in the reference's order, whose plan was made; -1: none             */
  int32_t slot;          /* the plan slot that holds its plan (navgpu_*_plans, navgpu_move_base_handover_plans); -1: none     */
  int32_t tried;         /* makePlan calls the reference would have made: winner + 1, or every candidate                      */
  int32_t n_candidates;  /* candidates of the request, the exact goal included                                                */
  int32_t n_poses;       /* poses of the winner's plan, the appended req.goal included; 0: none                               */
  int32_t rounds;        /* batches this request took part in                                                                 */
} navgpu_plan_service_result;
/* replaces: the candidate goals of planService (move_base.cpp:372-396) for one request, on the host: candidate 0 is the exact
 * goal; then, in float arithmetic as written (float resolution, search_increment = (float)(resolution * 3.0), replaced by
 * (float)tolerance when 0 < tolerance < search_increment; float loop variables compared with doubles; the max_offset - 1e-9 and
 * -1 * 0 skips), goal + (double)(offset * mult) for every ring.  out_xy = up to capacity x {x, y}; returns the number of
 * candidates (all of them, whatever the capacity), or NAVGPU_ERR_INVALID for NULL arguments or a resolution that is not positive
 * and finite.  The count stops at NAVGPU_PLAN_SERVICE_MAX_CANDIDATES + 1. */
int navgpu_move_base_plan_service_candidates(const double* goal_xy, double resolution, double tolerance, uint32_t capacity, double* out_xy);
/* replaces: planService's makePlan loop (move_base.cpp:365-417) for n_requests requests at once.  Request q owns the plan slots
 * [first_slot + q * slots_per_request, + slots_per_request) of the handle; their cost arrays must hold the request's costmap
 * (navgpu_navfn_set_costmap with shared = 1, or navgpu_navfn_set_costmap_from_fleet_instance, for the cost mode the family takes;
 * clearCostmapWindows (:363) is the caller's step before that, navgpu_move_base_clear_costmap_windows).  The candidates of each
 * request run through the family's make_plan (navgpu_global_planner_make_plan with params / options, or navgpu_navfn_ros_make_plan
 * with ros_params and the request's default_tolerance) slots_per_request at a time, every request of a round in one batch; a
 * request stops after the first round that holds a success, so with slots_per_request >= its candidates it is one batch.
 * The winner is the first candidate in the reference's order with status OK and n_poses > 0; when it is not candidate 0, req.goal
 * is appended to its plan (:402) by the emit pass: navgpu_*_plans and navgpu_move_base_handover_plans see the pose without a
 * host round trip.  winner_results (may be NULL) = n_requests x the family's make_plan result struct, the winner's (zeroed
 * without one; n_poses there does not count the appended pose).
 * Departure: the reference stops at the first success; here the candidates behind it in its round were planned too
 * (speculatively - their results are discarded, `tried` counts as the reference would).
 * NAVGPU_ERR_INVALID for NULL arguments, a bad range or family, what the family's make_plan refuses, or a request with more than
 * NAVGPU_PLAN_SERVICE_MAX_CANDIDATES candidates; nothing has run then. */
int navgpu_move_base_plan_service(navgpu_navfn* nav, uint32_t first_slot, uint32_t slots_per_request, uint32_t n_requests, int32_t family,
                                  const navgpu_global_planner_params* params, const navgpu_make_plan_options* options,
                                  const navgpu_navfn_ros_params* ros_params, const navgpu_plan_service_request* requests,
                                  navgpu_plan_service_result* results, void* winner_results);

/* ------------------------------------------------------------------------------------------ */
/* amcl::AMCLLaser - the laser sensor update of a batch of particle filters (one per robot)   */
/* ------------------------------------------------------------------------------------------ */
/* A handle holds n_filters independent particle filters ("filters") on one device: per filter a map (map_t), a sample set
 * (pf_sample_set_t: up to max_samples poses and weights and the converged flag), the pf_t running averages w_slow / w_fast
 * and the laser pose.  Filter k's samples live at k * max_samples in every sample array.  One laser model configuration
 * (navgpu_amcl_laser_configure) serves every filter of the handle.  All arithmetic is fp64 with the reference's operation
 * order; the device's libm (sin / cos / atan2 / exp / log) may differ from the host's by an ulp.  Coordinates are metres,
 * cells are map_t's (origin at the map centre, map.h:139-147).  Resampling, the kd-tree histogram and the cluster statistics
 * run on the device too (navgpu_amcl_update_resample below), and so does the odometry motion model (navgpu_amcl_update_action),
 * so a filter's set can stay on the device from one cycle to the next. */
typedef struct navgpu_amcl navgpu_amcl;
#define NAVGPU_AMCL_MODEL_BEAM 0                     /* laser_model_t, amcl_laser.h:42-48 */
#define NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD 1
#define NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD_PROB 2
#define NAVGPU_AMCL_MODEL_LIKELIHOOD_FIELD_GOMPERTZ 3
typedef struct {
  int32_t model_type;  /* NAVGPU_AMCL_MODEL_*                                                                              */
  int32_t max_beams;   /* AMCLLaser(max_beams, map); < 2: update_sensor returns updated = 0 and touches nothing             */
  /* SetModelBeam (amcl_laser.cpp:65-81) */
  double z_hit, z_short, z_max, z_rand, sigma_hit, lambda_short, chi_outlier;
  /* SetModelLikelihoodFieldProb (:100-120): the beam-skip parameters (z_hit, z_rand, sigma_hit as above; the max_occ_dist
   * argument of every SetModelLikelihoodField* is a property of the map: navgpu_amcl_set_map) */
  int32_t do_beamskip;
  int32_t reserved;
  double beam_skip_distance, beam_skip_threshold, beam_skip_error_threshold;
  /* SetModelLikelihoodFieldGompertz (:122-147) */
  double gompertz_a, gompertz_b, gompertz_c, input_shift, input_scale, output_shift;
  /* SetMapFactors (:149-156); the constructor's defaults are 1.0 / 1.0 / 0.0 (:51-53) */
  double off_map_factor, non_free_space_factor, non_free_space_radius;
  /* pf_alloc(..., alpha_slow, alpha_fast, ...) (pf.c:48-90) */
  double alpha_slow, alpha_fast;
} navgpu_amcl_laser_params;
/* replaces: pf_alloc / AMCLLaser::AMCLLaser (pf.c:48-90, amcl_laser.cpp:42-56) for n_filters filters.  max_beams is the
 * largest laser_params.max_beams the handle accepts (<= 1024); n_filters <= 65535 (NAVGPU_ERR_CAPACITY above). */
int navgpu_amcl_create(uint32_t n_filters, uint32_t max_samples, uint32_t max_beams, int32_t device, navgpu_amcl** out);
int navgpu_amcl_destroy(navgpu_amcl* amcl);
/* replaces: AmclNode::convertMap (amcl_node.cpp:1062-1093) + the map_update_cspace(map, max_occ_dist) call of
 * SetModelLikelihoodField* (amcl_laser.cpp:98,119,146).  occupancy = OccupancyGrid data, height x width (count of them, or
 * ONE map stored once for the whole slice when shared != 0); 0 -> free (-1), 100 -> occupied (+1), anything else -> unknown
 * (0); scale_up_factor in 1..16 (amcl_node.cpp:369-374) gives size = width * f x height * f, scale = resolution / f, and
 * origin_xy = {origin.position.x, .y} of the message (the same for every map of the call) is shifted to the map centre as
 * there.  size_x, size_y <= 16384.  The distance map is computed on the device as the EXACT capped Euclidean distance
 * transform: with D = the smallest squared cell distance (dx^2 + dy^2) to an occupied cell and R = (int)(max_occ_dist /
 * scale), a cell holds (float)max_occ_dist when sqrt((double)D) > R (or there is no occupied cell) and
 * (float)(sqrt((double)D) * scale) otherwise.  The reference's brushfire carries the source of whichever neighbour left its
 * priority queue first, which is order-dependent; it is never below the exact transform and above it on a few per cent of
 * cells (DESIGN "amcl").  navgpu_amcl_set_distance_map uploads the reference's own bytes. */
int navgpu_amcl_set_map(navgpu_amcl* amcl, uint32_t first, uint32_t count, const int8_t* occupancy, uint32_t width, uint32_t height,
                        double resolution, const double* origin_xy, int32_t scale_up_factor, int32_t shared, double max_occ_dist);
/* The same from a map_t as it stands (what an amcl::AMCLLaser holds): occ_state = size_y x size_x occ_state values (-1 free,
 * 0 unknown, +1 occupied) stored as given, scale and origin_x / origin_y (the map centre, map.h:63-67) taken as they are.
 * The distance map is computed as by navgpu_amcl_set_map. */
int navgpu_amcl_set_map_cells(navgpu_amcl* amcl, uint32_t first, uint32_t count, const int8_t* occ_state, uint32_t size_x, uint32_t size_y,
                              double scale, double origin_x, double origin_y, int32_t shared, double max_occ_dist);
/* map_t::distances as the caller computed them (e.g. the reference's map_update_cspace): size_y x size_x floats per filter
 * of the slice, or one array for all when shared != 0.  A map stored once for several filters of the slice takes the data
 * given for the last of them.  NAVGPU_ERR_STATE when a filter of the slice has no map. */
int navgpu_amcl_set_distance_map(navgpu_amcl* amcl, uint32_t first, uint32_t count, const float* distances, int32_t shared);
/* map_t::distances of one filter's map (size_y x size_x floats); NAVGPU_ERR_STATE when it has none */
int navgpu_amcl_distance_map(navgpu_amcl* amcl, uint32_t filter, float* out);
/* replaces: AMCLLaser::SetModelBeam / SetModelLikelihoodField / SetModelLikelihoodFieldProb / SetModelLikelihoodFieldGompertz /
 * SetMapFactors (amcl_laser.cpp:65-156) and pf_alloc's alpha_slow / alpha_fast.  All or nothing: an invalid struct
 * (model_type outside 0..3, max_beams outside 0..capacity - NAVGPU_ERR_CAPACITY above it -, do_beamskip not 0 / 1, a NaN
 * parameter) leaves the previous configuration in force. */
int navgpu_amcl_laser_configure(navgpu_amcl* amcl, const navgpu_amcl_laser_params* params);
/* replaces: AMCLLaser::SetLaserPose (amcl_laser.h:118): xyth = count x {x, y, theta} of the laser in the robot frame */
int navgpu_amcl_set_laser_pose(navgpu_amcl* amcl, uint32_t first, uint32_t count, const double* xyth);
/* pf_t::sets[current_set] of the slice: sample_counts[count] (<= max_samples, NAVGPU_ERR_CAPACITY above), poses = count x
 * max_samples x {x, y, theta} (pf_vector_t), weights = count x max_samples, converged[count].  Entries past a filter's
 * sample_count are stored and returned as given but take no part in an update.  get: any output pointer may be NULL.
 * set also sets each filter's kd-tree leaf count from its uploaded poses (navgpu_amcl_set_kd_leaf_counts). */
int navgpu_amcl_set_samples(navgpu_amcl* amcl, uint32_t first, uint32_t count, const int32_t* sample_counts, const double* poses,
                            const double* weights, const int32_t* converged);
int navgpu_amcl_get_samples(navgpu_amcl* amcl, uint32_t first, uint32_t count, int32_t* sample_counts, double* poses, double* weights,
                            int32_t* converged);
/* pf_t::w_slow, w_fast (pf.h:133): w = count x {w_slow, w_fast} */
int navgpu_amcl_set_filter_state(navgpu_amcl* amcl, uint32_t first, uint32_t count, const double* w);
int navgpu_amcl_get_filter_state(navgpu_amcl* amcl, uint32_t first, uint32_t count, double* w);
/* replaces: AMCLLaser::UpdateSensor -> pf_update_sensor(pf, ApplyModelToSampleSet, data) (amcl_laser.cpp:160-236, pf.c:270-316)
 * for every filter of the slice: the configured model, then (when its total is > 0) the map-factor pass, then normalisation
 * and the w_slow / w_fast running averages; weights become uniform when the total is 0.  The boundary is AMCLLaserData:
 * ranges_xy holds, filter after filter, range_counts[k] pairs {range, bearing} (laserReceived's ranges[i][0..1]),
 * range_max[k] per filter.  updated[k] = 1 where the update ran, 0 where the reference returns false (max_beams < 2; the
 * filter is untouched).  Sample totals are summed in a fixed order (not the reference's serial one: weights agree to a
 * relative 1e-12) that does not depend on the other filters.  Defined where the reference is not:
 * - the beam model's step (range_count - 1) / (max_beams - 1) is 0 for 1 <= range_count < max_beams and the reference's loop
 *   never ends (amcl_laser.cpp:265): such a filter gets updated[k] = NAVGPU_ERR_INVALID and is untouched, the others run and
 *   the call returns NAVGPU_ERR_INVALID;
 * - in the likelihood-field-prob model's beam skipping, the error branch (skipped beams >= max_beams * error threshold)
 *   integrates temp_obs[j][beam] for every beam < max_beams, including entries this update did not write (max-range / NaN
 *   beams and indices past the last subsampled beam: stale or uninitialised memory there).  Here only the entries written in
 *   this update are integrated, in both branches;
 * - the map factors read map_occ_dist even for the beam model, which needs no distances (the reference reads a NULL
 *   map_t::distances there unless something called map_update_cspace): here every map set by navgpu_amcl_set_map /
 *   _set_map_cells carries its exact distance map, whatever the model, so the factors are always defined.
 * NAVGPU_ERR_STATE for a filter without a map or before navgpu_amcl_laser_configure; nothing runs then.  A range_count above
 * INT32_MAX (AMCLLaserData::range_count is an int) is NAVGPU_ERR_INVALID. */
int navgpu_amcl_update_sensor(navgpu_amcl* amcl, uint32_t first, uint32_t count, const double* ranges_xy, const uint32_t* range_counts,
                              const double* range_max, int32_t* updated);
/* The likelihood-field-prob beam skipping of the last update of one filter (amcl_laser.cpp:543-566), arrays of the handle's
 * max_beams (navgpu_amcl_create) entries indexed by beam_ind: obs_count (particles whose beam end lies on the map closer than
 * beam_skip_distance to an obstacle), obs_mask (1: beam integrated) and *error (1: too many beams skipped, every written beam
 * integrated).  *active = 0 where the last update did not skip beams (do_beamskip off, set not converged, another model); the
 * rest is then zero.  Any output pointer may be NULL. */
int navgpu_amcl_beam_skip_state(navgpu_amcl* amcl, uint32_t filter, int32_t* obs_count, uint8_t* obs_mask, int32_t* error, int32_t* active);

/* ---- amcl resampling: pf_update_resample, the kd-tree histogram, pf_cluster_stats, pf_update_converged ---- */
#define NAVGPU_AMCL_RESAMPLE_MULTINOMIAL 0 /* pf_resample_model_t, pf.h */
#define NAVGPU_AMCL_RESAMPLE_SYSTEMATIC 1
#define NAVGPU_AMCL_DRAW_SUPPLIED 0 /* the caller's uniform draws and random poses (parity with the reference) */
#define NAVGPU_AMCL_DRAW_DEVICE 1   /* a counter-based generator on the device, seeded per call; nothing is uploaded */
typedef struct {
  int32_t resample_model; /* NAVGPU_AMCL_RESAMPLE_*                       pf_set_resample_model (pf.c:116-119)          */
  int32_t min_samples;    /* pf_alloc's min_samples (0 .. max_samples)                                                  */
  double pop_err, pop_z;  /* KLD bound, pf_alloc's 0.01 / 3 (pf.c:72-73; amcl_node's kld_err / kld_z)                  */
  double dist_threshold;  /* pf_update_converged's, 0.5 in pf_alloc (pf.c:74)                                          */
} navgpu_amcl_resample_params;
/* replaces: pf_set_resample_model and the pf_alloc fields above; max_samples is the handle's.  All or nothing: an invalid
 * struct (model not 0 / 1, min_samples outside 0..max_samples, pop_err not > 0, NaN) leaves the previous one in force. */
int navgpu_amcl_resample_configure(navgpu_amcl* amcl, const navgpu_amcl_resample_params* params);
/* replaces: pf_update_resample(pf) (pf.c:512-562) for every filter of the slice: draw set b from the current set, weights 1 / total,
 * w_slow = w_fast = 0 where w_diff > 0, the kd-tree histogram's leaf count, pf_cluster_stats and pf_update_converged (get_samples
 * returns the new set and its converged flag, get_clusters its clusters, get_kd_leaf_counts its leaf count).
 * draw_source NAVGPU_AMCL_DRAW_SUPPLIED: the reference's drand48() stream as values -
 *   multinomial: u = count x max_samples x {u_flag, u_pick}: candidate k is random when u_flag < w_diff, else the sample whose
 *     [c[i], c[i+1]) holds u_pick (u_pick of a random candidate is not read);
 *   systematic: systematic_start[count], systematic_sample_start;
 *   both: random_poses = the pools of the slice's filters one after the other, random_pose_counts[k] poses {x, y, theta} each,
 *     consumed in order (pf_t::random_pose_fn).  A pool shorter than the filter needs gives status[k] = NAVGPU_ERR_INVALID and
 *     the filter is untouched.  seed is not read.
 * draw_source NAVGPU_AMCL_DRAW_DEVICE: Philox4x32-10 keyed by `seed`, counter {draw, filter, the filter's call counter}; the
 *   call counter of every filter of the slice goes up by one per call (navgpu_amcl_set_rng_counters).  Random poses follow
 *   AmclNode::randomFreeSpacePose (amcl_node.cpp:1200-1212): a uniform index into the filter's map's free cells (occ_state -1,
 *   x-major, kept by navgpu_amcl_set_map*), the cell centre, theta = u * 2 pi - pi.  u, systematic_start, random_poses and
 *   random_pose_counts are not read.
 * The histogram key is floor(pose / {0.5, 0.5, 10 deg}) (pf_kdtree.c:72-74,116-118); the multinomial draw stops after candidate k
 * (1-based) once k > pf_resample_limit(leaf count of the first k); systematic draws pf_resample_limit(leaf count of the current
 * set AT ITS CREATION: set_samples / the previous resample / set_kd_leaf_counts) * (1 + w_diff) samples, the first
 * (int)(w_diff * new_count) of them random.  w_diff = 1 - w_fast / w_slow, clamped at 0.  Defined where the reference is not:
 * - a draw no interval [c[i], c[i+1]) holds (a systematic target in [c[n], 1.0] loops forever at pf.c:378-386, a multinomial
 *   u_pick >= c[n] reads samples[n] at pf.c:474-483; also u < 0 or NaN) picks the LAST SAMPLE WITH POSITIVE WEIGHT (sample n-1
 *   when no weight is positive);
 * - n_rand == new_count (w_diff == 1) makes every sample random; delta = 1 / 0 is never used;
 * - w_slow == 0 (0 / 0 or -inf after a reset) gives w_diff = 0, as the multinomial comparison with NaN does;
 * - a filter with sample_count 0, a random candidate without a pose (pool exhausted, a map without free cells), or a set b pose
 *   with a non-finite coordinate or |bin| > 2^20 - 2 gives status[k] = NAVGPU_ERR_INVALID and leaves that filter untouched.
 * Weights of set a must be >= 0 (as update_sensor leaves them).  Clusters are numbered by their lowest sample index (the
 * reference numbers them in kd-tree node order, which depends on the insertion history); none is dropped.  Sums run in
 * sample order in one lane, so two runs give identical bytes.  Returns NAVGPU_ERR_INVALID when any filter failed (the others
 * ran), NAVGPU_ERR_STATE before navgpu_amcl_resample_configure or for device draws on a filter without a map. */
int navgpu_amcl_update_resample(navgpu_amcl* amcl, uint32_t first, uint32_t count, int32_t draw_source, const double* u,
                                const double* systematic_start, const double* random_poses, const uint32_t* random_pose_counts, uint64_t seed,
                                int32_t* status);
/* replaces: pf_get_cluster_stats (pf.c:760-779) and the set's cluster_count read at amcl_node.cpp:1590-1597 for the current set
 * of one filter after a resample: *cluster_count, then for the first min(cluster_count, capacity) clusters counts[k], weights[k],
 * means[k][3], covs[k][3][3]; set_mean[3], set_cov[9] are pf_sample_set_t::mean / cov.  Any array may be NULL.
 * NAVGPU_ERR_CAPACITY when cluster_count > capacity (the first `capacity` are written); NAVGPU_ERR_STATE (cluster_count 0)
 * before the filter's first resample. */
int navgpu_amcl_get_clusters(navgpu_amcl* amcl, uint32_t filter, int32_t* cluster_count, uint32_t capacity, int32_t* counts,
                             double* weights, double* means, double* covs, double* set_mean, double* set_cov);
/* pf_kdtree_t::leaf_count of each filter's current set as it was created, what systematic resampling sizes set b from
 * (pf.c:342).  navgpu_amcl_set_samples sets it from the uploaded poses, as pf_init_model's inserts do (pf.c:180-205);
 * update_resample sets it to the new set's. */
int navgpu_amcl_set_kd_leaf_counts(navgpu_amcl* amcl, uint32_t first, uint32_t count, const int32_t* leaf_counts);
int navgpu_amcl_get_kd_leaf_counts(navgpu_amcl* amcl, uint32_t first, uint32_t count, int32_t* leaf_counts);
/* The device generator's per-filter call counters (0 at create); with the same seed, counter and set a call repeats its draws. */
int navgpu_amcl_set_rng_counters(navgpu_amcl* amcl, uint32_t first, uint32_t count, const uint64_t* counters);
int navgpu_amcl_get_rng_counters(navgpu_amcl* amcl, uint32_t first, uint32_t count, uint64_t* counters);

/* ---- amcl odometry motion model: AMCLOdom::UpdateAction -> pf_update_action ---- */
#define NAVGPU_AMCL_ODOM_DIFF 0 /* odom_model_t, amcl_odom.h:38-45, same order */
#define NAVGPU_AMCL_ODOM_OMNI 1
#define NAVGPU_AMCL_ODOM_DIFF_CORRECTED 2
#define NAVGPU_AMCL_ODOM_OMNI_CORRECTED 3
#define NAVGPU_AMCL_ODOM_GAUSSIAN 4
#define NAVGPU_AMCL_DRAW_DRAND48 2 /* the reference's drand48() stream, regenerated on the device from its state */
typedef struct {
  int32_t model_type;                         /* NAVGPU_AMCL_ODOM_*                                                    */
  int32_t reserved;
  double alpha1, alpha2, alpha3, alpha4, alpha5; /* SetModel's drift parameters (alpha5: omni and Gaussian only)       */
} navgpu_amcl_odom_params;
/* replaces: AMCLOdom::SetModelDiff / SetModelOmni / SetModelGaussian / SetModel (amcl_odom.cpp:68-125).  All or nothing: a
 * model outside 0..4 or a NaN alpha leaves the previous configuration in force.  Negative alphas are accepted as in the reference:
 * the uncorrected models then draw with a negative "stddev", the corrected ones with sqrt of a negative (NaN). */
int navgpu_amcl_odom_configure(navgpu_amcl* amcl, const navgpu_amcl_odom_params* params);
/* replaces: AMCLOdom::UpdateAction(pf, data) (amcl_odom.cpp:128-379) for every filter of the slice.  odom = count x 9 doubles:
 * AMCLOdomData's pose[3], delta[3], absolute_motion[3] as amcl_node.cpp:1444-1464 fills them (absolute_motion is read by the
 * Gaussian model only).  Every sample < sample_count of each filter moves in place; nothing else changes: weights, converged,
 * w_slow / w_fast, the clusters of the last resample, the kd-tree leaf count (pf_update_action rebuilds no tree, and systematic
 * resampling sizes from the count "as created") and the entries past sample_count.  theta is not normalised (as in the
 * reference).  Everything that depends on the odometry alone (delta_rot1 / delta_trans / delta_rot2, the *_noise terms, the
 * stddevs, angle_diff(atan2(dy, dx), old_theta), normalize(delta_rot1 / delta_rot2)) is computed on the host with the host's
 * libm in the reference's own expressions; per particle the device's sin / cos / atan2 / log may differ from the host's by an ulp
 * (angle_diff and normalize are atan2(sin(z), cos(z)), so a 1-ulp difference can wrap a result near +-pi by 2 pi).
 * A Gaussian deviate is pf_ran_gaussian's (pf_pdf.c:132-146), multiplied left to right as C parses it:
 *   (sigma * x2) * sqrt(-2.0*log(w)/w).
 * draw_source NAVGPU_AMCL_DRAW_DRAND48 (parity with the reference): drand48_state[k] is filter k's 48-bit LCG state X, in and
 *   out (after srand48(s) it is (s & 0xFFFFFFFF) << 16 | 0x330E; the next drand48() is ((0x5DEECE66D X + 0xB) mod 2^48) / 2^48).
 *   Each filter draws 3 deviates per sample in sample order and in each model's own order (diff: rot1, trans, rot2; omni: trans,
 *   rot, strafe; Gaussian: trans, strafe, rot): values equal to 0.0 are skipped, the others are paired consecutively as
 *   (x1, x2) = 2 r - 1, and a pair is accepted when 0 < w = x1*x1 + x2*x2 <= 1.  The state comes back advanced by exactly the
 *   number of values the reference's loop consumes.  A state >= 2^48 gives status[k] = NAVGPU_ERR_INVALID and leaves that filter
 *   (and its state) untouched.  seed is not read.
 * draw_source NAVGPU_AMCL_DRAW_DEVICE: Philox4x32-10 keyed by `seed` (see update_resample), counter {draw, filter | 2 << 16,
 *   the filter's call counter}: sample i takes the two double pairs (u0, u1) of draw 2 i and (u2, u3) of draw 2 i + 1 (53-bit
 *   doubles in [0, 1)) and its three deviates, in the model's order, are
 *     r0 = sqrt(-2 log(1 - u0)), z0 = r0 * cos(2 pi u1), z1 = r0 * sin(2 pi u1), z2 = sqrt(-2 log(1 - u2)) * cos(2 pi u3),
 *   each used as pf_ran_gaussian's value: sigma * z.  The call counter is the one update_resample uses and goes up by one per
 *   call for every filter of the slice, so consecutive motion and resample calls never repeat draws.  drand48_state is not read.
 * Any other draw_source (NAVGPU_AMCL_DRAW_SUPPLIED included) is NAVGPU_ERR_INVALID.  NAVGPU_ERR_STATE before
 * navgpu_amcl_odom_configure (no map is needed); NAVGPU_ERR_INVALID for a NULL odom or a NULL drand48_state in drand48 mode, and
 * when any filter failed (the others ran). */
int navgpu_amcl_update_action(navgpu_amcl* amcl, uint32_t first, uint32_t count, const double* odom, int32_t draw_source,
                              uint64_t* drand48_state, uint64_t seed, int32_t* status);

/* ---- amcl filter initialisation: pf_init and pf_init_model (global localisation) ---- */
/* Both calls leave each filter's set as pf_init leaves it: sample_count = the handle's max_samples, every weight 1.0 / max_samples,
 * w_slow = w_fast = 0, converged 0, the kd-tree leaf count = the number of distinct histogram bins of the new set, and the
 * clusters and set mean / cov of pf_cluster_stats, numbered by lowest sample index as after update_resample (get_clusters is
 * valid right after an init).  draw_source is NAVGPU_AMCL_DRAW_DRAND48 or NAVGPU_AMCL_DRAW_DEVICE, with update_action's
 * conventions: drand48_state[k] in and out (not read in device mode), the device call counter +1 per call for every filter
 * that ran (shared with update_action / update_resample).  status[k] per filter; a filter that fails is untouched, its drand48
 * state included, and so are the filters outside the slice.  A pose that is not finite or has |bin| > 2^20 - 2 fails the filter
 * with NAVGPU_ERR_INVALID (a negative eigenvalue of cov, whose sqrt the reference takes, gives NaN poses). */
/* replaces: pf_init(pf, mean, cov) (pf.c:138-176) with pf_pdf_gaussian_alloc / _sample (pf_pdf.c:46-126).  mean = count x 3,
 * cov = count x 9 (row-major).  The host decomposes cov as pf_matrix_unitary does (Householder tridiagonalisation and QL
 * iteration, fp64, the same operation order): rotation cr and cd[j] = sqrt(eigenvalue j), eigenvalues ascending.  Per sample
 * r[j] = pf_ran_gaussian(cd[j]) for j = 0, 1, 2, then x[i] = mean[i] + cr[i][0] r[0] + cr[i][1] r[1] + cr[i][2] r[2], left to right.
 * drand48: the 3 max_samples deviates of update_action's drand48 mode, in sample order; pass the state srand48(++pf_pdf_seed)
 *   leaves, (seed << 16) | 0x330E.  Device: Philox stream 3, counter {draw, filter | 3 << 16, call counter}; sample i takes draws
 *   2 i and 2 i + 1 and update_action's Box-Muller deviates z0, z1, z2, each scaled as cd[j] * z.
 * NAVGPU_ERR_INVALID for NULL arguments or when any filter failed (a non-finite mean or cov, a state >= 2^48, a bad pose). */
int navgpu_amcl_init_gaussian(navgpu_amcl* amcl, uint32_t first, uint32_t count, const double* mean, const double* cov,
                              int32_t draw_source, uint64_t* drand48_state, uint64_t seed, int32_t* status);
typedef struct {
  double starting_weight_threshold; /* uniform_pose_starting_weight_threshold                                        */
  double deweight_multiplier;       /* uniform_pose_deweight_multiplier                                              */
  uint64_t max_candidates;          /* per filter per call; 0 = 100 x max_samples; at most 2^40, 2^32 with device draws */
} navgpu_amcl_uniform_params;
/* replaces: pf_init_model(pf, AmclNode::uniformPoseGenerator, node) (pf.c:180-213, amcl_node.cpp:1200-1263).  A candidate is
 * randomFreeSpacePose over the filter's free cells: cells with occ_state -1 and map_occ_dist > the configured
 * non_free_space_radius (0 before navgpu_amcl_laser_configure), x-major as amcl_node.cpp:1026-1033 lists them; the cell centre
 * and theta = u * 2 pi - pi.  Candidates are scored only when a scan is given (ranges_xy, range_counts and range_max as in
 * update_sensor; ranges_xy == NULL && range_counts == NULL means last_laser_data_ == NULL), starting_weight_threshold > 0 and
 * 0 <= deweight_multiplier < 1 (amcl_node.cpp:1253).  The score is scorePose's: the configured laser model on a one-sample set of
 * weight 1.0, converged 0 (no beam skipping), subsampled as update_sensor does, with the filter's laser pose; then the map
 * factors when it is > 0.  A sample retries while score < gw, gw *= deweight_multiplier after every retry; gw restarts at the
 * threshold for every sample; a NaN score accepts.
 * drand48: candidate j of a filter takes values 2 j (cell) and 2 j + 1 (theta) of its stream (no zero skipping); the state comes
 *   back advanced by 2 x candidates_used[k].  Device: Philox stream 4, counter {sample, filter | 4 << 16, call counter (its low 32
 *   bits), retry}: each sample runs its own retry sequence, distributed as the reference's draws, not its stream.
 *   Every candidate drawn counts towards the filter's total at once, and all its samples stop when the total passes
 *   max_candidates, so a call draws at most about max_candidates + max_samples candidates per filter.
 * candidates_used[k] (may be NULL): the candidates drawn (max_samples when unscored).  Defined where the reference is not:
 * - a map without free cells gives status[k] = NAVGPU_ERR_INVALID;
 * - a filter that needs more than max_candidates candidates gets status[k] = NAVGPU_ERR_CAPACITY.  The reference loops as long as
 *   it takes (forever when no candidate can reach the decayed threshold, e.g. with negative scores);
 * - the beam model with 1 <= range_count < max_beams (the reference's loop never ends) gives NAVGPU_ERR_INVALID.
 * Returns NAVGPU_ERR_CAPACITY when a filter hit the cap, else NAVGPU_ERR_INVALID when any filter failed (the others ran);
 * NAVGPU_ERR_STATE for a filter without a map or a scan before navgpu_amcl_laser_configure (nothing runs then). */
int navgpu_amcl_init_uniform(navgpu_amcl* amcl, uint32_t first, uint32_t count, const navgpu_amcl_uniform_params* params,
                             const double* ranges_xy, const uint32_t* range_counts, const double* range_max, int32_t draw_source,
                             uint64_t* drand48_state, uint64_t seed, uint64_t* candidates_used, int32_t* status);

/* ---- amcl node: AmclNode::laserReceived for every filter of a slice, one call per scan ---- */
/* A ROS-free mirror of what AmclNode keeps and decides between scans (amcl/src/amcl_node.cpp:1316-1756), one laser per filter
 * (lasers_update_ is one flag).  The pf steps are the calls above, with device draws; here they are chained for the whole slice
 * with each filter predicated by what the node decides for it, and the call waits for the device once.  The tf look-ups stay
 * with the caller (getOdomPose's result and the two tf::getYaw results of the scan's first two rays are inputs), as does every
 * message.  tf's 3-D arithmetic is restated in its planar form, not pinned. */
typedef struct {
  double d_thresh, a_thresh;      /* update_min_d / update_min_a (amcl_node.cpp:1403-1412)                                 */
  double laser_min_range;         /* <= 0: unset, the message's range_min holds (amcl_node.cpp:1518-1522)                  */
  double laser_max_range;         /* <= 0: unset (amcl_node.cpp:1514-1517)                                                 */
  int32_t resample_interval;      /* >= 1 (amcl_node.cpp:1546)                                                             */
  int32_t use_odom_integrator;    /* odom_integrator_topic_.size() != 0 (amcl_node.cpp:1403, 1454)                         */
} navgpu_amcl_node_params;
/* replaces: the node's parameters read at amcl_node.cpp:1403-1412, 1514-1522, 1546.  All or nothing: NAVGPU_ERR_INVALID for a
 * NaN, resample_interval < 1 (the reference would compute % 0) or use_odom_integrator outside {0, 1}; the configuration in
 * force stays then. */
int navgpu_amcl_node_configure(navgpu_amcl* amcl, const navgpu_amcl_node_params* params);
#define NAVGPU_AMCL_SCAN_PRESENT 1u /* navgpu_amcl_scan::flags bit 0: a LaserScan arrived for this filter in this call */
typedef struct {
  uint32_t flags;                 /* NAVGPU_AMCL_SCAN_PRESENT; a filter without it is untouched, its node state included   */
  uint32_t range_count;           /* laser_scan->ranges.size()                                                             */
  uint32_t range_offset;          /* first range of this filter in the call's `ranges` array                               */
  float range_min, range_max;     /* the message's floats                                                                  */
  uint32_t reserved;
  double yaw_min, yaw_inc;        /* tf::getYaw(min_q), tf::getYaw(inc_q) after transformQuaternion (amcl_node.cpp:1505-1506) */
  double odom_pose[3];            /* getOdomPose's x, y, yaw at the scan's stamp (amcl_node.cpp:1383)                      */
} navgpu_amcl_scan;
typedef struct {
  int32_t status;                 /* NAVGPU_OK; NAVGPU_ERR_INVALID: the filter was refused and is untouched (see below)    */
  int32_t moved;                  /* AMCLOdom::UpdateAction ran (amcl_node.cpp:1442-1470)                                  */
  int32_t updated;                /* the sensor step ran: the `if (lasers_update_[laser_index])` block (:1474-1582)        */
  int32_t resampled;              /* pf_update_resample ran (:1546-1549)                                                   */
  int32_t cloud_due;              /* the particle cloud would be published: `if (!m_force_update)` (:1562) inside that block */
  int32_t published;              /* max_weight > 0.0 (:1614): pose, covariance and map_to_odom below are this scan's      */
  int32_t republish;              /* the `else if (latest_tf_valid_)` branch (:1726): latest_tf_ is sent again              */
  int32_t global_localization_converged; /* global_localization_active_ was cleared by this call (:1550-1554)              */
  int32_t sample_count, converged;/* the current set after the call                                                        */
  int32_t cluster_count;          /* hypotheses read (0 unless resampled or force_publication)                             */
  int32_t max_weight_hyp;         /* -1 when none has weight > 0                                                           */
  double max_weight;
  double pose[3];                 /* hyps[max_weight_hyp].pf_pose_mean                                                     */
  double cov_xx, cov_xy, cov_yx, cov_yy, cov_aa; /* set->cov.m[0][0], [0][1], [1][0], [1][1], [2][2] (:1637-1651)         */
  double map_to_odom[3];          /* x, y, theta of latest_tf_.inverse() (:1708): what is broadcast global -> odom          */
} navgpu_amcl_node_result;
/* replaces: AmclNode::laserReceived from getOdomPose's result on (amcl_node.cpp:1381-1756) for filters first .. first + count - 1.
 * scans = count records; ranges = every flagged filter's raw LaserScan::ranges as floats (a filter reads range_count of them at
 * range_offset; the call uploads max(range_offset + range_count) floats); results = count records, zeroed for a filter
 * without NAVGPU_AMCL_SCAN_PRESENT.  Per flagged filter, in the reference's order:
 * - delta = pose - pf_odom_pose_ with angle_diff on the yaw (:1397-1399, the host's libm); update = |delta x|, |delta y| > d_thresh
 *   or |delta yaw| > a_thresh, or with use_odom_integrator sqrt(abs x^2 + abs y^2) >= d_thresh or abs yaw >= a_thresh over the
 *   integrator's absolute motion (:1403-1412); update |= m_force_update and m_force_update is cleared, only inside if (pf_init_);
 * - a filter with pf_init_ false takes the first-scan branch (:1423-1440): pf_odom_pose_ = pose, lasers_update_, resample_count_ = 0,
 *   the integrator not ready, force_publication; a pending nomotion request survives it and forces the next scan's update;
 * - otherwise, with lasers_update_, UpdateAction with odata.pose / delta / absolute_motion (:1447-1464: navgpu_amcl_update_action's
 *   9 doubles) and the integrator's absolute motion is zeroed (:1469);
 * - with lasers_update_: the scan is converted (:1505-1537): angle_increment = fmod(yaw_inc - yaw_min + 5 pi, 2 pi) - pi on the
 *   host; range_max = min(msg range_max, (float)laser_max_range) and range_min = max(msg range_min, (float)laser_min_range) as
 *   floats when set, then widened; on the device (k_amcl_scan), only for the rays the model's subsampling step reads:
 *   range = (double)ranges[i] <= range_min ? range_max : ranges[i] (a NaN passes through), bearing = angle_min + (i * angle_increment)
 *   with the product rounded before the sum: the bytes of a host-built AMCLLaserData.  Then UpdateSensor, lasers_update_ = false,
 *   pf_odom_pose_ = pose; when !(++resample_count_ % resample_interval) the resample, and global_localization_active_ is
 *   cleared when the resampled filter is converged (:1546-1555);
 * - when resampled or force_publication the hypotheses are read (:1584-1651, navgpu_amcl_hypotheses below) and, with
 *   max_weight > 0, latest_tf_ is set; else with latest_tf_valid_ the result says republish.
 * map_to_odom: for the hypothesis h and the scan's odometry pose o, theta = h.theta - o.theta, (x, y) = h.xy - R(theta) o.xy, the
 *   planar form of :1678-1700 computed on the host; latest_tf_ (navgpu_amcl_node_get_state) is its inverse, {-R(-theta) xy, -theta}.
 *   This restates tf's 3-D quaternion arithmetic and is not pinned to it: expect its rounding to differ in the last bits.
 * Draws are the device generator's (NAVGPU_AMCL_DRAW_DEVICE) keyed by `seed`; a filter's call counter goes up by one for each
 * of UpdateAction and the resample that ran for it, and by none otherwise: the bytes are those of navgpu_amcl_update_action,
 * navgpu_amcl_update_sensor and navgpu_amcl_update_resample called for that filter alone, in this order, with the same seed.
 * With laser max_beams < 2 UpdateSensor returns false in the reference (amcl_laser.cpp:163-164) and nothing of the sensor step
 * runs on the device; the node's bookkeeping (updated, resample_count_) goes on as in the reference.
 * One call enqueues the motion model, the conversion, the sensor model, the resample and the read-out for the slice back to
 * back and waits once; nothing of a step's result is read by the host in between.
 * NAVGPU_ERR_STATE before navgpu_amcl_node_configure, navgpu_amcl_laser_configure, navgpu_amcl_odom_configure or
 * navgpu_amcl_resample_configure, or for a flagged filter without a map: nothing runs and no state changes.  A flagged filter
 * whose beam model would loop forever (1 <= range_count < max_beams, amcl_laser.cpp:265), whether or not its update is due, gets
 * status = NAVGPU_ERR_INVALID and is untouched, node state included; the others run and the call returns NAVGPU_ERR_INVALID,
 * as it does when a resample fails a filter (status = that code; navgpu_amcl_update_resample). */
int navgpu_amcl_node_laser_received(navgpu_amcl* amcl, uint32_t first, uint32_t count, const navgpu_amcl_scan* scans,
                                    const float* ranges, uint64_t seed, navgpu_amcl_node_result* results);
/* replaces: the hypothesis read-out of amcl_node.cpp:1584-1651 alone, for every filter of the slice, from whatever clusters the
 * last resample or init left (k_amcl_hypothesis, one read-back for the slice).  This is what force_publication reads right
 * after an init.  Fills cluster_count, max_weight_hyp, max_weight, published, pose, the covariance entries, sample_count and
 * converged; the other fields are 0 (map_to_odom needs a scan's odometry pose).  The hypothesis is the first cluster with the
 * strictly largest weight in the device's cluster order (clusters are numbered by their lowest sample index, get_clusters):
 * with exactly equal weights the reference's kd-tree order may pick another cluster.  A filter that was never resampled or
 * initialised reports published = 0, cluster_count = 0. */
int navgpu_amcl_hypotheses(navgpu_amcl* amcl, uint32_t first, uint32_t count, navgpu_amcl_node_result* results);
typedef struct {
  int32_t pf_init;                       /* pf_init_                                                                      */
  int32_t lasers_update;                 /* lasers_update_[0] (true when the laser is first seen, amcl_node.cpp:1344)     */
  int32_t force_update;                  /* m_force_update                                                                */
  int32_t resample_count;                /* resample_count_                                                               */
  int32_t odom_integrator_ready;         /* odom_integrator_ready_                                                        */
  int32_t global_localization_active;    /* global_localization_active_                                                   */
  int32_t latest_tf_valid;               /* latest_tf_valid_                                                              */
  int32_t reserved;
  double pf_odom_pose[3];                /* pf_odom_pose_                                                                 */
  double odom_integrator_absolute_motion[3]; /* odom_integrator_absolute_motion_                                          */
  double odom_integrator_last_pose[3];   /* odom_integrator_last_pose_                                                    */
  double latest_tf[3];                   /* latest_tf_ as planar x, y, theta (odom -> global)                             */
} navgpu_amcl_node_state;
/* Host-only, no device work.  replaces: what applyInitialPose (amcl_node.cpp:1862-1876) and globalLocalizationCallback
 * (:1265-1293) do to the node after the init call the caller makes itself: pf_init_ = false, and
 * global_localization_active_ = global_localization != 0. */
int navgpu_amcl_node_reset(navgpu_amcl* amcl, uint32_t first, uint32_t count, int32_t global_localization);
/* replaces: AmclNode::nomotionUpdateCallback (amcl_node.cpp:1296-1303): m_force_update = true */
int navgpu_amcl_node_request_nomotion_update(navgpu_amcl* amcl, uint32_t first, uint32_t count);
/* replaces: AmclNode::integrateOdom (amcl_node.cpp:1120-1172) for one odometry message per filter of the slice, in the
 * reference's own expressions with the host's libm.  poses = count x {x, y, yaw} of the message (getEulerYPR's yaw is the
 * caller's).  NAVGPU_ERR_INVALID for a NULL argument. */
int navgpu_amcl_node_integrate_odom(navgpu_amcl* amcl, uint32_t first, uint32_t count, const double* poses);
/* Every member the mirror keeps, per filter of the slice (checkpointing, tests) */
int navgpu_amcl_node_get_state(navgpu_amcl* amcl, uint32_t first, uint32_t count, navgpu_amcl_node_state* states);
int navgpu_amcl_node_set_state(navgpu_amcl* amcl, uint32_t first, uint32_t count, const navgpu_amcl_node_state* states);

/* ------------------------------------------------------------------------------------------ */
/* costmap_3d::Costmap3DQuery - batched mesh-vs-occupancy collision and distance queries      */
/* ------------------------------------------------------------------------------------------ */
/* A handle of its own (as navgpu_navfn): n_instances resident 3-D occupancy maps of one size and one robot mesh.  A map is a
 * dense bit volume: one uint64_t per (x, y) column, bit z set when cell (x, y, z) is occupied, in two planes per instance -
 * LETHAL and NONLETHAL, the reference's "strictly between FREE and LETHAL" (costmap_3d/include/costmap_3d/costmap_3d.h:48-60).
 * Cell (i, j, k) is the closed cube [origin + (i, j, k) * resolution, origin + (i + 1, j + 1, k + 1) * resolution].
 * What a query computes is geometry: the robot is the closed solid bounded by the mesh at the pose, the obstacles are
 * the closed cubes of the occupied cells.  It is what the reference's octree / BVH solver and interior-collision look-up table
 * approximate (costmap_3d/src/costmap_3d_query.cpp:586-939); FCL's own answers are not pinned.
 * The device is opened by the first call that needs it (NAVGPU_ERR_NO_DEVICE there, never a CPU fallback): every argument error
 * below is found before that, and before anything is queued.  Calls on one handle are serialised and ordered on one stream. */
typedef struct navgpu_costmap3d navgpu_costmap3d;
#define NAVGPU_C3D_MAX_TRIANGLES 384 /* largest max_triangles: a pose's world triangles live in one workgroup's LDS */
typedef struct {
  uint32_t n_instances;
  uint32_t size_x, size_y; /* columns; size_x * size_y <= 2^26                                                  */
  uint32_t size_z;         /* levels, 1..64                                                                     */
  double resolution;       /* edge of a cell, > 0                                                               */
  uint32_t max_triangles;  /* 1..NAVGPU_C3D_MAX_TRIANGLES                                                       */
  uint32_t max_boxes;      /* per navgpu_costmap3d_set_boxes call                                               */
  uint32_t max_poses;      /* per query call (and its runs)                                                     */
  int32_t device;
} navgpu_costmap3d_desc;
typedef struct {
  double cx, cy, cz; /* centre                                                                                  */
  double size;       /* edge: resolution * 2^k (an octomap leaf of any depth)                                   */
  int32_t cls;       /* NAVGPU_C3D_LETHAL | NAVGPU_C3D_NONLETHAL                                                */
  int32_t reserved;
} navgpu_c3d_box;
typedef struct {
  uint32_t instance;
  uint32_t first_pose; /* index into the call's pose array                                                      */
  uint32_t n_poses;
} navgpu_c3d_run;
typedef struct {
  double cost;          /* distance mode: the minimum over the run's poses, from DBL_MAX; else the fold below  */
  int32_t n_lethal;     /* poses with a negative cost (response.lethal_indices.size())                         */
  int32_t first_lethal; /* index within the run of the first of them, -1 when there is none                    */
  int32_t n_done;       /* poses answered: n_poses, or with lazy first_lethal + 1                               */
  int32_t reserved;
} navgpu_c3d_run_result;
enum { NAVGPU_C3D_LETHAL = 0, NAVGPU_C3D_NONLETHAL = 1 };
enum { NAVGPU_C3D_REPLACE = 0, NAVGPU_C3D_MARK = 1, NAVGPU_C3D_CLEAR = 2 };
/* GetPlanCost3D.srv's numbers; COST_QUERY_MODE_SIGNED_DISTANCE (3) is NAVGPU_ERR_INVALID: the reference's own README calls it not functional */
enum { NAVGPU_C3D_COST = 0, NAVGPU_C3D_COLLISION_ONLY = 1, NAVGPU_C3D_DISTANCE = 2 };
enum { NAVGPU_C3D_REGION_ALL = 0, NAVGPU_C3D_REGION_LEFT = 1, NAVGPU_C3D_REGION_RIGHT = 2, NAVGPU_C3D_REGION_RECTANGULAR_PRISM = 3 };

/* replaces: Costmap3DQuery::Costmap3DQuery / init (costmap_3d/src/costmap_3d_query.cpp:58-126) for n_instances maps.  Host only:
 * NAVGPU_ERR_INVALID for a NULL argument, a zero count, size_z > 64, size_x * size_y > 2^26, a resolution that is not positive
 * and finite, max_triangles > NAVGPU_C3D_MAX_TRIANGLES or a negative device.  Origins start at (0, 0, 0), the maps empty. */
int navgpu_costmap3d_create(const navgpu_costmap3d_desc* desc, navgpu_costmap3d** out);
int navgpu_costmap3d_destroy(navgpu_costmap3d* c3d);
/* replaces: the octree's fixed frame (Costmap3DQuery::checkCostmap, costmap_3d_query.cpp:138-287, reads the tree in the costmap's
 * frame): the world position of the corner of cell (0, 0, 0) of one instance.  Not finite: NAVGPU_ERR_INVALID. */
int navgpu_costmap3d_set_origin(navgpu_costmap3d* c3d, uint32_t instance, const double origin_xyz[3]);
int navgpu_costmap3d_get_origin(navgpu_costmap3d* c3d, uint32_t instance, double origin_xyz[3]);
/* replaces: Costmap3DQuery::updateCostmap (costmap_3d_query.cpp:128-136; mode REPLACE: the boxes are the whole map) and the
 * deltas of an octomap update that checkCostmap (:138-287) follows (MARK, CLEAR).  A box is an octomap leaf of any depth: size
 * must be resolution * 2^k and the box aligned to the instance's grid (both to 1e-6 of a cell), else NAVGPU_ERR_INVALID with the
 * map untouched; so for a cls outside the two, a non-finite field and a bad mode.  n > max_boxes: NAVGPU_ERR_CAPACITY.  A pruned
 * leaf is rasterised into its finest cells (the union of closed cubes is the same set); cells outside the extents are dropped
 * and counted in clipped_out (or NULL).  MARK sets the cells in the plane of cls and clears them in the other plane, CLEAR
 * clears them in both (cls is not looked at); one call must not name a cell in both classes (an octomap leaf has one value).
 * k_c3d_rasterize: vector atomicOr / atomicAnd on the column words, which commute - the result does not depend on the order. */
int navgpu_costmap3d_set_boxes(navgpu_costmap3d* c3d, uint32_t instance, int32_t mode, const navgpu_c3d_box* boxes, uint32_t n,
                               uint32_t* clipped_out);
/* Raw access to an instance's planes (tests, checkpoints; as navgpu_grid_upload / navgpu_grid_download - no reference lines, the
 * reference keeps an octomap::OcTree, costmap_3d.h:48-60 names the classes): size_y * size_x words each, word index y * size_x + x.
 * Either pointer may be NULL (that plane is skipped); a bit at or above size_z in an upload is NAVGPU_ERR_INVALID. */
int navgpu_costmap3d_columns_upload(navgpu_costmap3d* c3d, uint32_t instance, const uint64_t* lethal, const uint64_t* nonlethal);
int navgpu_costmap3d_columns_download(navgpu_costmap3d* c3d, uint32_t instance, uint64_t* lethal, uint64_t* nonlethal);
/* replaces: Costmap3DQuery::updateMeshResource (costmap_3d_query.cpp:413-449) with padPoints (costmap_3d/include/costmap_3d/
 * costmap_3d_query.h:332-350: every vertex pushed radially in xy by `padding`, the arithmetic in float as written there, the
 * origin left alone).  vertices = nv x {x, y, z}, triangles = nt x 3 vertex indices.  closed_out (or NULL) says whether the mesh
 * is closed and consistently oriented - every directed edge has its opposite exactly once.  An open mesh is treated as a
 * surface: there is no interior test for it.  nt > max_triangles: NAVGPU_ERR_CAPACITY.  NAVGPU_ERR_INVALID for nt == 0, an index
 * >= nv, a coordinate or padding that is not finite, or a triangle without area.  A call that fails leaves the previous mesh. */
int navgpu_costmap3d_set_mesh(navgpu_costmap3d* c3d, const double* vertices, uint32_t nv, const uint32_t* triangles, uint32_t nt,
                              double padding, int32_t* closed_out);
/* replaces: Costmap3DROS::processPlanCost3D (costmap_3d/src/costmap_3d_ros.cpp:464-616) over Costmap3DQuery::footprintCollision /
 * footprintCost / footprintDistance (costmap_3d_query.cpp:493-521, 586-970) for n_runs runs of poses, each against one instance:
 * one upload, one launch set (k_c3d_query: a wave per pose; k_c3d_fold: a lane per run), one read-back.
 *   runs       any instances in any order, an instance more than once; their pose ranges must not overlap (NAVGPU_ERR_INVALID)
 *              and must end at or below max_poses, n_runs <= max_poses (NAVGPU_ERR_CAPACITY)
 *   poses      {x, y, z, qx, qy, qz, qw} per pose; the quaternion is normalised on the device; a pose that is not finite or has
 *              a zero quaternion is NAVGPU_ERR_INVALID
 *   mode       NAVGPU_C3D_COST | _COLLISION_ONLY | _DISTANCE
 *   regions    per pose, or NULL (ALL): the half-spaces of RegionsOfInterestAtPose (costmap_3d_query.h:573-617) at the pose, the
 *              prism with region_scale[1] and [2].  A cell is considered unless it lies entirely outside some half-space - centre
 *              distance minus extent > 0, checkROI (costmap_3d/include/costmap_3d/octree_solver.h:248-285) - per finest cell
 *   obstacles  per pose, or NULL (LETHAL): honoured in distance mode only, as in the reference (costmap_3d_ros.cpp:533-551)
 * Per pose: it collides iff a considered occupied cell's closed cube intersects a mesh triangle, or - closed mesh - the centre of
 * one lies inside the solid (winding number from the triangles' solid angles, |w| > 0.5).  COLLISION_ONLY and COST (the
 * reference's TODO, costmap_3d_query.cpp:493-497): -1.0 | 0.0.  DISTANCE: -1.0 when colliding, else the Euclidean distance between
 * the mesh and the considered occupied cells closer than distance_limit, else distance_limit as given (DBL_MAX for an empty map,
 * an empty region, a pose off the extents); a limit <= 0 is raised to DBL_MIN (costmap_3d_query.cpp:632).
 * Per run: the fold of costmap_3d_ros.cpp:494-609 in results_out (or NULL).  With lazy a run ends at its first lethal pose and
 * pose_costs_out (or NULL; indexed as poses) behind it is left untouched. */
int navgpu_costmap3d_query(navgpu_costmap3d* c3d, uint32_t n_runs, const navgpu_c3d_run* runs, const double* poses, int32_t mode,
                           const uint8_t* regions, const uint8_t* obstacles, const double region_scale[3], double distance_limit,
                           int32_t lazy, double* pose_costs_out, navgpu_c3d_run_result* results_out);
/* replaces: base_local_planner::Costmap3DModel::footprintCost(x, y, theta, ...) (base_local_planner/src/costmap_3d_model.cpp:61-79):
 * the pose is (x, y, 0) with the yaw quaternion, the query the cost mode over ALL.  poses_xyth = {x, y, theta} per pose, indexed by
 * the runs as above; costs_out one double per pose and first_illegal_out (or NULL) per run the index within it of the first
 * negative cost, -1 when there is none - navgpu_footprint_cost's layout. */
int navgpu_costmap3d_footprint_costs(navgpu_costmap3d* c3d, uint32_t n_runs, const navgpu_c3d_run* runs, const double* poses_xyth,
                                     double* costs_out, int32_t* first_illegal_out);

/* The handle's layered map update from point clouds and its projection into 2-D: configure_layers, layer_set,
 * buffer_clouds, set_static_grid, update, reset, layer2d_download, layer2d_update_costs and the layers' raw column access. */
#include "navgpu_costmap3d_layers.h"
/* Rolling 3-D maps and the reset of a bounding box: the two calls that move or clear what the layers hold. */
#include "navgpu_costmap3d_rolling.h"
/* The maps' way out of a handle and into a layer: pruned octree leaves, Costmap3DPublisher and updateCells. */
#include "navgpu_costmap3d_publish.h"

#ifdef __cplusplus
}
#endif
#endif /* NAVGPU_H_ */
