/* navgpu_costmap3d rolling: a handle's 3-D maps follow their robots, and the reset of a bounding box.  Included by
 * navgpu.h, after navgpu_costmap3d_layers.h; do not include this file on its own.
 *
 * A rolling costmap_3d map keeps its cells at world-fixed keys: when the window moves, each layer deletes what lies outside the
 * rolled box without tracking the deletion (costmap_3d/src/costmap_layer_3d.cpp:56-65), LayeredCostmap3D::updateMap drops the
 * out-of-box entries of its bounds map (costmap_3d/src/layered_costmap_3d.cpp:123) and the master loses what lies outside the box
 * (:140-145).  Here a map is a window of size_x x size_y columns at an integer key origin, so a roll by (dx, dy) cells sends the
 * column that was at (x, y) to (x - dx, y - dy): columns that leave are forgotten, columns that enter are empty - absent in every
 * plane - until a layer puts something there.  z does not roll (costmap_3d/include/costmap_3d/layer_3d.h:125-131).
 *
 * The static 3-D layer does not come back by itself: Static2DLayer3D fills its tree once per grid message
 * (static_2d_layer_3d.cpp:201-299) and its updateBounds is the base class's, so a column that re-enters the window is empty in
 * that layer too.  The caller sends navgpu_costmap3d_set_static_grid again when it wants the layer refilled.
 *
 * Stated differences from the reference:
 *  - The maximum edge.  The reference deletes with deleteAABB of the octomap fork it builds against; a box whose corners are not
 *    on the lattice may keep one more column at the maximum edge there than this window of exactly size columns holds.
 *  - The 2-D bounds after a move.  The reference's addExtraBounds(getOriginX(), getOriginY(), getSizeInMetersX(),
 *    getSizeInMetersY()) (costmap_3d_to_2d_layer.cpp:120-127) passes sizes where maxima belong; here the bounds are the window,
 *    {ox, oy, ox + size_x * res, oy + size_y * res}.
 *  - Clipping of clouds.  The reference clips a cloud at the update that follows it; navgpu_costmap3d_buffer_clouds clips against
 *    the window of its own moment.  So a cycle is roll, then buffer_clouds, then update: a cell that was outside the old window
 *    when it was buffered is absent until the next cloud, even if a roll brings it inside.
 * A cylinder layer's previous set is kept as (pose, radius) in world coordinates; the next update evaluates it against the new
 * window, so a roll has nothing to do for it. */
#ifndef NAVGPU_COSTMAP3D_ROLLING_H_
#define NAVGPU_COSTMAP3D_ROLLING_H_

enum { NAVGPU_C3D_ROLL_CENTRE = 0, NAVGPU_C3D_ROLL_ORIGIN = 1 };

/* replaces: LayeredCostmap3D::updateMap's rolling window (costmap_3d/src/layered_costmap_3d.cpp:77-94, 120-145) with
 * CostmapLayer3D::updateBounds' deletion (costmap_layer_3d.cpp:56-65) and Costmap3DTo2DLayer's origin change
 * (costmap_3d_to_2d_layer.cpp:117-127), for a list of distinct instances in one launch set (k_c3d_roll_y, k_c3d_roll_x,
 * k_c3d_roll_bits) behind whatever is queued on the handle's stream; the call returns queued, as navgpu_costmap3d_reset does.
 * targets_xy = {x, y} per listed instance.
 *   NAVGPU_C3D_ROLL_CENTRE  the robot's position.  Per axis, as updateMap computes it with octomap::point3d's floats (:78-92):
 *                           w = (double)(float)(size * resolution), m = (float)(robot - w / 2.0), and the window's first key is
 *                           (int64)floor((double)m * (1.0 / resolution)).
 *   NAVGPU_C3D_ROLL_ORIGIN  the new origin, a multiple of the resolution to 1e-6 of a cell (the layer calls' test): what
 *                           navgpu_fleet_get_origin returns for a rolling 2-D fleet, whose origin Costmap3DTo2DLayer must share.
 * The window is the size columns from that key and the instance's origin becomes key * resolution in x and y (z is kept); the host's
 * and the device's copy follow in stream order, so navgpu_costmap3d_get_origin and navgpu_costmap3d_query see it afterwards.
 * shifts_out (or NULL) holds {dx, dy} per listed instance, in cells.  An instance whose shift is (0, 0) is not touched (its
 * origin neither) and gets no moved mark.  |dx| >= size_x or |dy| >= size_y empties the instance's data, the changed planes too
 * (this is not the full flag).  On a handle without navgpu_costmap3d_configure_layers the master's LETHAL and NONLETHAL planes are
 * shifted; on a layered handle the master's three planes, every costmap layer's current planes and changed plane (changed_cells_ is
 * world-keyed) and the 2-D layer's bytes, entering columns NO_INFORMATION - the projection is a function of the master column, so
 * these are the bytes of the reference's full re-projection.  The moved mark makes the instance's next navgpu_costmap3d_update
 * report the whole window as its 2-D bounds; its 3-D bounds are not widened.  navgpu_costmap3d_reset and
 * navgpu_costmap3d_configure_layers clear the mark (the full flag implies it).
 * NAVGPU_ERR_INVALID, found on the host before anything is queued and with nothing changed: a NULL handle, an instance out of range
 * or listed twice, an unknown mode, a target that is not finite, in ORIGIN mode an unaligned target, a current origin that is
 * unaligned, or a key beyond 2^30 in magnitude. */
int navgpu_costmap3d_roll(navgpu_costmap3d* c3d, uint32_t n, const uint32_t* instances, int32_t mode,
                          const double* targets_xy /* n x {x, y}: robot position or new origin */,
                          int32_t* shifts_out /* n x {dx, dy} cells, or NULL */);
/* replaces: Costmap3DROS::resetBoundingBox (costmap_3d/src/costmap_3d_ros.cpp:270-303) over CostmapLayer3D::resetBoundingBox
 * (costmap_layer_3d.cpp:149-191) for a list of distinct instances in one launch (k_c3d_reset_box); returns queued.  boxes =
 * {min x, y, z, max x, y, z} per listed instance; layer_mask bit l names layer l.  In each named POINT_CLOUD layer the cells whose
 * key lies between coordToKey(min) and coordToKey(max), both ends inclusive per axis as in the reference's key loops, clipped to
 * the window, are deleted and added to the layer's changed plane; the next update recombines them.  A box with min > max on any
 * axis, or wholly outside the window, deletes nothing.  A STATIC_2D layer ignores the call (static_2d_layer_3d.cpp:153-158), so
 * its mask bit is accepted and does nothing.  So is a cylinder layer's - a stated difference: the reference forgets the part of
 * the previous clearing set inside the box (cylinder_clearing_layer_3d.cpp:174-197); here the set is a pose and a radius, and
 * keeping it only widens the next update's bounds.  NAVGPU_ERR_STATE before configure_layers; NAVGPU_ERR_INVALID for an instance
 * out of range or listed twice, a layer_mask bit beyond the configured layers, a box that is not finite or an unaligned origin. */
int navgpu_costmap3d_reset_bounding_box(navgpu_costmap3d* c3d, uint32_t n, const uint32_t* instances,
                                        const double* boxes /* n x {min xyz, max xyz} */, uint32_t layer_mask);

#endif /* NAVGPU_COSTMAP3D_ROLLING_H_ */
