/* navgpu_costmap3d layers: the per-cycle producer of a navgpu_costmap3d handle's maps.  Included by navgpu.h, which
 * declares the handle and the status codes; do not include this file on its own.
 *
 * costmap_3d rebuilds its 3-D map from sensor data every cycle: PointCloudLayer3D replaces its layer by the cells of the newest
 * cloud, Static2DLayer3D places the static map at one height, CylinderClearingLayer3D erases a cylinder round the robot,
 * LayeredCostmap3D::updateMap recombines the changed cells into the master tree and Costmap3DTo2DLayer projects the changed
 * columns into a costmap_2d layer.  Here that runs for a batch of instances on the bit volumes of the handle.
 *
 * A cell is absent (the reference's missing node), FREE, NONLETHAL or LETHAL, held one-hot in three planes of uint64_t column
 * words.  The master keeps its LETHAL and NONLETHAL planes where navgpu_costmap3d_query reads them and gains a FREE plane; a
 * POINT_CLOUD or STATIC_2D layer has three planes of its own and a `changed` plane per instance (CostmapLayer3D::changed_cells_).
 * Difference from the reference: NONLETHAL carries no value.  The order is absent < FREE < NONLETHAL < LETHAL and
 * the 2-D cost of a NONLETHAL column is the handle parameter nonlethal_cost_2d (default 127: toCostmap2D of Cost 0.0, the
 * midpoint, costmap_3d/plugins/costmap_3d_to_2d_layer.cpp:279-288).
 *
 * The layer calls need an instance origin that is a multiple of the resolution to 1e-6 of a cell (navgpu_costmap3d_set_boxes'
 * alignment test), else NAVGPU_ERR_INVALID.  With ok = llround(origin / resolution) per axis, the cell of a coordinate c is
 * (int64)floor(c * (1.0 / resolution)) - ok (octomap's coordToKey, which multiplies by resolution_factor) and a cell centre is
 * ((double)(ok + i) + 0.5) * resolution (keyToCoord).  Everything is integers, bits, bytes, or fp64 under -ffp-contract=off.
 *
 * Every argument error is found on the host before the device is opened and before anything is queued; a call that fails
 * changes nothing resident.  A handle on which navgpu_costmap3d_configure_layers is never called allocates and behaves as
 * before.  navgpu_costmap3d_set_boxes and navgpu_costmap3d_columns_upload keep writing the master directly: on a layered handle
 * the next update rebuilds whatever lies inside its bounds from the layers, and leaves the rest as those calls wrote it. */
#ifndef NAVGPU_COSTMAP3D_LAYERS_H_
#define NAVGPU_COSTMAP3D_LAYERS_H_

#define NAVGPU_C3D_MAX_LAYERS 8
enum { NAVGPU_C3D_LAYER_POINT_CLOUD = 0, NAVGPU_C3D_LAYER_STATIC_2D = 1, NAVGPU_C3D_LAYER_CYLINDER_CLEARING = 2 };
/* costmap_3d/cfg/GenericPlugin.cfg's numbers */
enum { NAVGPU_C3D_COMBINE_OVERWRITE = 0, NAVGPU_C3D_COMBINE_MAXIMUM = 1, NAVGPU_C3D_COMBINE_IF_UNKNOWN = 2, NAVGPU_C3D_COMBINE_NOTHING = 99 };
typedef struct {
  int32_t kind;               /* NAVGPU_C3D_LAYER_*                                                                 */
  int32_t enabled;
  int32_t combination_method; /* NAVGPU_C3D_COMBINE_* (costmap layers; a cylinder layer ignores it)                 */
  int32_t cloud_has_intensity;   /* POINT_CLOUD: points are xyzi (pcl::PointXYZI), else xyz and every point LETHAL     */
  float free_intensity;          /* POINT_CLOUD with intensity                                                          */
  float lethal_intensity;
  int32_t lethal_cost_threshold; /* STATIC_2D: 0..255 (a uint8_t in the reference)                                      */
  int32_t unknown_to_lethal;     /* STATIC_2D                                                                           */
  double height;                 /* STATIC_2D: the level is the cell of this z                                          */
  double radius;                 /* CYLINDER_CLEARING: its absolute value is used                                       */
  uint32_t max_cloud_points;     /* POINT_CLOUD: points of one navgpu_costmap3d_buffer_clouds call (the largest counts) */
  uint32_t reserved;
} navgpu_c3d_layer;
typedef struct {
  uint32_t instance;
  uint32_t layer;
  uint32_t first_point; /* index of the cloud's first point in the call's point array                           */
  uint32_t n_points;
  double transform[12]; /* row-major 3 x 3 basis, then the origin: the cloud's frame in the map's                */
} navgpu_c3d_cloud;

/* replaces: LayeredCostmap3D::addPlugin and sizeChange (costmap_3d/src/layered_costmap_3d.cpp:245-330), the layers' parameters
 * (point_cloud_layer_3d.cpp:60-98, static_2d_layer_3d.cpp:63-104, cylinder_clearing_layer_3d.cpp:52-76) and
 * Costmap3DTo2DLayer::matchSize (costmap_3d_to_2d_layer.cpp:100-112).  Every plane is empty afterwards, the 2-D layer is
 * NO_INFORMATION, and every instance's next update treats the whole map as changed (size_changed_, copy_full_map_).  A second
 * call reconfigures from scratch.  The largest max_cloud_points bounds the points of one navgpu_costmap3d_buffer_clouds call.
 * NAVGPU_ERR_INVALID for n_layers == 0 or > NAVGPU_C3D_MAX_LAYERS, an unknown kind or combination method, intensities that are
 * not finite or equal, a threshold outside 0..255, a height or radius that is not finite, nonlethal_cost_2d outside 0..255 or a
 * POINT_CLOUD layer with max_cloud_points == 0. */
int navgpu_costmap3d_configure_layers(navgpu_costmap3d* c3d, const navgpu_c3d_layer* layers, uint32_t n_layers, int32_t nonlethal_cost_2d);
/* replaces: Static2DLayer3D::reconfigureCallback's touch (static_2d_layer_3d.cpp:106-134): when enabled or combination_method
 * changes, every present cell of a costmap layer is marked changed in every instance.  A stated superset of the reference:
 * PointCloudLayer3D::reconfigureCallback (point_cloud_layer_3d.cpp:100-112) forgets to touch.  A cylinder layer only takes the
 * values.  NAVGPU_ERR_STATE before configure_layers; NAVGPU_ERR_INVALID for a bad layer index or method. */
int navgpu_costmap3d_layer_set(navgpu_costmap3d* c3d, uint32_t layer, int32_t enabled, int32_t combination_method);
/* replaces: PointCloudLayer3D::pointCloudCallback (point_cloud_layer_3d.cpp:171-243) for many (instance, layer) pairs in one
 * upload and one launch set (k_c3d_cloud: a lane per point, vector atomicOr on the column words - OR commutes, the planes do
 * not depend on point order; k_c3d_layer_swap).  points holds n_points records of 3 floats (xyz) or 4 (xyzi), by the layers'
 * cloud_has_intensity: every layer named in one call must have the same format.  Per point: transform in fp64 as
 * r0*x + r1*y + r2*z + t, left to right, rounded to float as PCL stores it; the class from the float Cost of
 * pointIntensityToCost (:159-169, in float as written): LETHAL when >= 10, FREE when <= -10, else NONLETHAL; the cell as above.
 * A point that is not finite or lies outside the extents is dropped and counted per cloud in clipped_out (or NULL).  Per cell
 * the highest class wins (:210-214).  The layer becomes exactly the cloud's cells (the net effect of erase_cells,
 * unchanged_cells and markAndClearCells, :218-241) and changed |= old ^ new over the three planes; across calls the changed
 * bits accumulate until an update consumes them.  NAVGPU_ERR_INVALID for two clouds of one (instance, layer) pair in one call,
 * a layer that is no POINT_CLOUD layer, mixed formats, a point range beyond n_points, a transform that is not finite or an
 * unaligned origin; NAVGPU_ERR_CAPACITY for n_points > max_cloud_points; NAVGPU_ERR_STATE before configure_layers. */
int navgpu_costmap3d_buffer_clouds(navgpu_costmap3d* c3d, const navgpu_c3d_cloud* clouds, uint32_t n_clouds, const float* points,
                                   uint32_t n_points, uint32_t* clipped_out);
/* replaces: Static2DLayer3D::occupancyGridCallback (static_2d_layer_3d.cpp:189-299) for one (instance, layer): the class of
 * occupancyGridToCost (:189-199; an unknown cell without unknown_to_lethal makes no cell), the cell of each grid cell's centre
 * origin + i * resolution + resolution / 2.0 at level coordToKey(height), and the replace-and-diff of buffer_clouds
 * (k_c3d_static2d, k_c3d_layer_swap).  The grid's resolution is the map's.  Cells off the extents are dropped and counted in
 * clipped_out (or NULL).  NAVGPU_ERR_INVALID for a layer that is no STATIC_2D layer, a zero size, width * height > 2^26, an
 * origin that is not finite or an unaligned instance origin. */
int navgpu_costmap3d_set_static_grid(navgpu_costmap3d* c3d, uint32_t instance, uint32_t layer, const int8_t* occupancy, uint32_t width,
                                     uint32_t height, double origin_x, double origin_y, uint32_t* clipped_out);
/* replaces: LayeredCostmap3D::updateMap (layered_costmap_3d.cpp:60-165; its rolling part is navgpu_costmap3d_roll), for a list of distinct instances in one
 * launch set (k_c3d_combine: a lane per column word), with CostmapLayer3D::updateBounds / updateCosts (costmap_layer_3d.cpp:
 * 51-108), CylinderClearingLayer3D::updateBounds / updateCosts (cylinder_clearing_layer_3d.cpp:78-160) and
 * Costmap3DTo2DLayer::updateFrom3D / updateBounds (costmap_3d_to_2d_layer.cpp:114-277).  robot_poses_xyz = {x, y, z} per listed
 * instance.  bounds is the OR of the layers' changed planes (then cleared) and of every cylinder layer's previous and current
 * clearing sets - the current set is the columns in the clamped key box of pose +- radius whose centre satisfies
 * x*x + y*y <= r*r, over all levels; it then becomes the previous one; a disabled cylinder layer forgets its previous set after
 * adding it.  An instance whose full flag is set (configure, reset) uses everything as bounds.  Inside bounds the master is
 * erased and the enabled layers applied in order - Overwrite: a present layer cell replaces the master cell (FREE replaces
 * LETHAL too); Maximum: the higher class wins; IfUnknown: only where the master is absent; Nothing; a cylinder layer erases its
 * current set.  Outside bounds the master does not change.  For every column with a bounds bit the 2-D layer's byte becomes 254
 * if any LETHAL bit is set, else nonlethal_cost_2d if any NONLETHAL bit, else 0 if any FREE bit, else 255 (the reference
 * re-projects a bounding box; the projection is a function of the master column, so the results are equal), and the 2-D bounds
 * are extended by origin + x0*res, origin + y0*res, origin + (x1+1)*res, origin + (y1+1)*res.  bounds2d_out (or NULL) holds
 * {min_x, min_y, max_x, max_y} per listed instance, {1e6, 1e6, -1e6, -1e6} when empty (costmap_2d/src/costmap_layer.cpp:55-58);
 * the pending bounds are consumed (useExtraBounds).  An instance whose window moved since its last update (navgpu_costmap3d_roll's
 * moved mark, which this call consumes) reports the whole window, {ox, oy, ox + size_x * res, oy + size_y * res}.
 * NAVGPU_ERR_INVALID for an instance out of range or listed twice, a pose that is not finite or an unaligned origin. */
int navgpu_costmap3d_update(navgpu_costmap3d* c3d, uint32_t n, const uint32_t* instances, const double* robot_poses_xyz, double* bounds2d_out);
/* replaces: LayeredCostmap3D::reset (layered_costmap_3d.cpp:183-194) for the listed instances: the master and every costmap
 * layer are cleared with their changed planes, cylinder layers forget their previous set, the full flag is set. */
int navgpu_costmap3d_reset(navgpu_costmap3d* c3d, uint32_t n, const uint32_t* instances);
/* replaces: Costmap3DTo2DLayer's costmap_ (costmap_3d_to_2d_layer.cpp:196-232): the window [x0, xn) x [y0, yn) of an instance's
 * 2-D layer, (yn - y0) rows of (xn - x0) bytes. */
int navgpu_costmap3d_layer2d_download(navgpu_costmap3d* c3d, uint32_t instance, uint32_t x0, uint32_t y0, uint32_t xn, uint32_t yn, uint8_t* out);
/* replaces: Costmap3DTo2DLayer::updateCosts (costmap_3d_to_2d_layer.cpp:238-244) - CostmapLayer::updateWithMax (use_maximum) or
 * updateWithOverwrite (costmap_2d/src/costmap_layer.cpp:62-124) - over the cell box [min_i, max_i) x [min_j, max_j) of
 * boxes_ij = {min_i, min_j, max_i, max_j} per listed instance, into instance i of a resident byte grid the caller names: what
 * navgpu_grid_device(fleet, NAVGPU_GRID_MASTER, ...) returns.  size_x and size_y must equal the 3-D map's columns and every
 * listed instance lie below grid_instances, else NAVGPU_ERR_INVALID; so for a box outside the grid.  The call returns after
 * the work is done; it runs on this handle's stream, so the caller keeps the handle that owns the grid idle meanwhile. */
int navgpu_costmap3d_layer2d_update_costs(navgpu_costmap3d* c3d, uint32_t n, const uint32_t* instances, void* device_grid,
                                          size_t instance_stride_bytes, uint32_t grid_instances, uint32_t size_x, uint32_t size_y,
                                          const int32_t* boxes_ij, int32_t use_maximum);
/* Raw access for tests and checkpoints (as navgpu_costmap3d_columns_download; the reference keeps octomap trees,
 * costmap_3d/include/costmap_3d/costmap_3d.h:48-60 names the classes): a costmap layer's planes and its changed plane, and the
 * master's FREE plane; size_y * size_x words each, any pointer may be NULL. */
int navgpu_costmap3d_layer_columns_download(navgpu_costmap3d* c3d, uint32_t instance, uint32_t layer, uint64_t* lethal, uint64_t* nonlethal,
                                            uint64_t* free_cells, uint64_t* changed);
int navgpu_costmap3d_free_columns_download(navgpu_costmap3d* c3d, uint32_t instance, uint64_t* free_cells);

#endif /* NAVGPU_COSTMAP3D_LAYERS_H_ */
