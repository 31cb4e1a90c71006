/* navgpu_costmap3d publishing: a handle's 3-D maps leave as pruned octree leaves and enter a layer as such.  Included by
 * navgpu.h, after navgpu_costmap3d_rolling.h; do not include this file on its own.
 *
 * The lattice.  A leaf's key is its minimum corner on the signed cell lattice, floor(coord / resolution) per axis.  With the layer
 * calls' ok = llround(origin / resolution), cell (i, j, k) of a window has lattice index ok + (i, j, k).  A leaf of level L is the
 * cube of 2^L cells per axis and its key is a multiple of 2^L on every axis (floor-mod for negative keys) - octomap's own
 * alignment, whose key offset 2^(depth-1) is a multiple of every 2^L.  size_z <= 64, so level <= 6.  Origins must be aligned as for
 * the layer calls, and a window whose lattice indices do not fit int32_t is NAVGPU_ERR_INVALID.
 *
 * Canonical pruning, as octomap's prune() leaves a tree: a node becomes a leaf iff all its 8 children are leaves of the same class;
 * level-0 leaves are the present cells; the output is the set of maximal leaves.  A node with a child outside the window cannot be
 * full - nothing exists there - so window edges need no rule of their own.
 *
 * Order of an export's leaves (positions come from counts and scans, never from an atomic counter: two calls on the same state
 * give identical bytes): by listed instance; then by 64 x 64-column lattice-aligned block, row-major (block y, then block x); in
 * the values array then by class (LETHAL, NONLETHAL, FREE); then by level, coarse to fine; then by key y, key x, key z.
 *
 * Stated differences from the reference:
 *  - The bounds of a DELTA.  The reference's bounds_map is the union of the layers' changed_cells_, the cylinders' sets and what
 *    left the box (costmap_3d/src/layered_costmap_3d.cpp:96-164); it may hold cells whose value did not change.  The bounds here
 *    are the cells of the window whose master class differs from the master as last published (the shadow) - the subset that
 *    changed.  A subscriber that applies either ends with the same map.  So writes that bypass the layers (set_boxes,
 *    columns_upload), navgpu_costmap3d_reset and rolls are published too.
 *  - What left the window is sent as at most two lattice boxes (forgotten), not as bounds leaves.
 *  - Value cells outside the bounds.  navgpu_costmap3d_layer_update_cells ignores them; the octomap fork that defines
 *    setTreeValues is not at hand to say what it does with them.
 *  - NAVGPU_C3D_CELLS_AS_GIVEN is a superset of the reference's import, which knows binary maps only. */
#ifndef NAVGPU_COSTMAP3D_PUBLISH_H_
#define NAVGPU_COSTMAP3D_PUBLISH_H_

enum { NAVGPU_C3D_FREE = 2 };                  /* third leaf class, beside NAVGPU_C3D_LETHAL / _NONLETHAL */
typedef struct { int32_t key[3]; uint16_t level; uint16_t cls; } navgpu_c3d_leaf;   /* 16 bytes */

enum { NAVGPU_C3D_EXPORT_FULL = 0, NAVGPU_C3D_EXPORT_DELTA = 1 };
enum { NAVGPU_C3D_CELLS_BINARY = 0, NAVGPU_C3D_CELLS_AS_GIVEN = 1 };
enum { NAVGPU_C3D_APPLIED = 0, NAVGPU_C3D_IGNORED = 1, NAVGPU_C3D_RESYNC = 2 };
typedef struct {
  uint32_t instance;
  uint32_t update_seq, bounds_seq;
  int32_t  universe;            /* the bounds are everything: no bounds leaves, no forgotten boxes            */
  int32_t  plain_map;           /* import only: a `costmap_3d` topic message (mapCallback), no sequence logic */
  uint32_t first_value, n_values, first_bound, n_bounds;   /* ranges in the call's arrays; counts always true */
  uint32_t n_forgotten;         /* 0..2                                                                       */
  int32_t  forgotten[2][6];     /* lattice boxes min xyz, max xyz, inclusive                                  */
} navgpu_c3d_update_msg;        /* 88 bytes */

/* replaces: Costmap3DPublisher's constructor and its update_seq_ (costmap_3d/src/costmap_3d_publisher.cpp:46-70), for every
 * instance of the handle.  Host state only; the device buffers come with the first DELTA export.  enabled != 0: every instance
 * gets a shadow - the master as last published, three planes on a layered handle, two without layers - the lattice window the
 * shadow was taken at, and an update_seq that starts at 0.  Shadows start empty and without a window (so the first DELTA forgets
 * nothing).  Calling it again reconfigures from scratch; enabled == 0 drops the state.  On a handle where it is never called
 * nothing is allocated and nothing behaves differently.  NAVGPU_ERR_INVALID for a NULL handle. */
int navgpu_costmap3d_publisher_configure(navgpu_costmap3d* c3d, int32_t enabled);

/* replaces: Costmap3DPublisher::connectCallback / createMapMessage (costmap_3d_publisher.cpp:77-93, 113-122) as mode FULL and
 * updateCompleteCallback / createMapUpdateMessage (costmap_3d_publisher.cpp:95-111, 124-154) as mode DELTA, behind
 * LayeredCostmap3D::updateMap's delta (layered_costmap_3d.cpp:156-164), for a list of distinct instances: one upload and one
 * launch set (k_c3d_export counting, k_c3d_export_scan, k_c3d_export emitting, for DELTA k_c3d_shadow_copy), a read-back of the counts
 * and one of the leaves.  msgs[i] describes instances[i]; its ranges index values / bounds, where the listed instances' leaves
 * stand behind one another in list order.
 *   FULL   the values are the whole master, pruned per class; universe = 1, no bounds leaves; bounds_seq = update_seq - 1 in
 *          uint32_t arithmetic, the reference's sentinel for a first map; update_seq and the shadow do not change.  Works without
 *          publisher_configure: both sequence numbers are then 0 (no publisher, no sentinel: feed such a message to
 *          navgpu_costmap3d_layer_update_cells as a plain_map).
 *   DELTA  needs publisher_configure (NAVGPU_ERR_STATE).  The bounds are the window's cells whose master class differs from the
 *          shadow's - read at the cell's world-fixed lattice position, absent outside the shadow's window - pruned as one binary
 *          plane (cls LETHAL); the values are the master's present cells inside the bounds, pruned per class.  forgotten covers
 *          shadow window \ current window as at most two lattice boxes over the shadow window's z range: first the x strip over
 *          the old y range, then the y strip over the remaining x range.  Both sequence numbers are update_seq.  On success the
 *          shadow becomes the master, its window the current one, and update_seq increments - for an empty delta too: the
 *          reference publishes every cycle.
 * Capacities, in leaves.  If either total exceeds its capacity the call returns NAVGPU_ERR_CAPACITY with every msgs[i] filled in
 * (counts and ranges as they would be) and commits nothing: no shadow and no sequence number moves.  values = bounds = NULL with
 * zero capacities counts only - NAVGPU_OK, msgs filled in - and commits nothing either.
 * NAVGPU_ERR_INVALID, found on the host before anything is queued: a NULL handle or msgs, an instance out of range or listed
 * twice, a mode that is neither, a NULL buffer with a capacity, an unaligned origin or a window beyond int32_t.  A call that
 * needs the device on a machine without one returns NAVGPU_ERR_NO_DEVICE (n = 0 needs none). */
int navgpu_costmap3d_export(navgpu_costmap3d* c3d, uint32_t n, const uint32_t* instances, int32_t mode, uint32_t value_capacity,
                            navgpu_c3d_leaf* values, uint32_t bounds_capacity, navgpu_c3d_leaf* bounds, navgpu_c3d_update_msg* msgs);

/* replaces: CostmapLayer3D::updateCells (costmap_3d/src/costmap_layer_3d.cpp:216-242) under OctomapServerLayer3D's mapCallback,
 * mapUpdateCallback and mapUpdateInternal (costmap_3d/plugins/octomap_server_layer_3d.cpp:281-434), for a list of messages to
 * distinct (instance, layer) pairs in one upload and one launch set (k_c3d_cells_raster, k_c3d_cells_resolve).  msgs[i].instance
 * is the destination instance and layers[i] its layer: any costmap layer (POINT_CLOUD or STATIC_2D; an OctomapServerLayer3D is a
 * POINT_CLOUD layer with max_cloud_points = 1 that is fed by this call instead of clouds).  The ranges of msgs[i] index values
 * (n_values leaves) and bounds (n_bounds leaves).
 * Per applied message, with W the destination window: E = the cells of the bounds leaves (everything when universe or plain_map,
 * as mapCallback passes no bounds) plus the forgotten boxes, clipped to W.  The layer becomes (old & ~E) | (V & E), V the cells
 * of the value leaves by class - setTreeValues(value, bounds, false, true): erase inside the bounds, then set.  A value cell
 * outside E is ignored.  Where two value leaves of one message name a cell in different classes the higher class wins (LETHAL
 * over NONLETHAL over FREE), whatever the leaf order.  changed |= E: the whole bounds, not the diff (touch(bounds_map), :241).
 * cell_mode NAVGPU_C3D_CELLS_BINARY is the reference's rule for an incoming binary map with threshold 0
 * (octomap_server_layer_3d.cpp:427-428): an occupied leaf (cls LETHAL or NONLETHAL) becomes LETHAL, FREE stays FREE;
 * NAVGPU_C3D_CELLS_AS_GIVEN keeps the three classes.  The layer's current plane set stays current; its occupancy bits cover
 * every tile that holds a cell (a superset, as after reset_bounding_box), a tile with a changed bit has its dirty bit, the next
 * scratch set stays empty.  The call returns queued.
 * Subscription state per (instance, layer), on the host, as mapUpdateCallback keeps it (:288-350); verdicts_out[i] (or NULL):
 *   NAVGPU_C3D_APPLIED
 *   NAVGPU_C3D_IGNORED  the first message since (re)subscription is a normal update (bounds_seq == update_seq); or a plain_map
 *                       message once updates are in use (:284)
 *   NAVGPU_C3D_RESYNC   a second message arrives without a first full map - also right after an ignored one, as in the reference -
 *                       or last_seq + 1 < bounds_seq in uint32_t: the state is reset as subscribeUpdatesUnlocked does (:179-186)
 *                       and the caller fetches a FULL export.
 * A sequence number that moves backwards is applied (:333-339).  Messages with another verdict than APPLIED queue nothing, and
 * neither does an applied one without a cell inside the window (an empty delta), so a call of such messages needs no device.  navgpu_costmap3d_configure_layers resets every pair's state.
 * NAVGPU_ERR_STATE before configure_layers.  NAVGPU_ERR_CAPACITY for n_values + n_bounds > max_boxes.  NAVGPU_ERR_INVALID for a
 * NULL handle, msgs or layers, an unknown cell_mode, an instance or layer out of range, a cylinder layer, a pair named twice, a
 * key not aligned to its level, level > 6, a class that is none of the three, ranges beyond the arrays, n_forgotten > 2, a
 * forgotten box with max < min, or an unaligned origin.  A failing call changes nothing resident and no subscription state. */
int navgpu_costmap3d_layer_update_cells(navgpu_costmap3d* c3d, uint32_t n_msgs, const navgpu_c3d_update_msg* msgs, const uint32_t* layers,
                                        int32_t cell_mode, const navgpu_c3d_leaf* values, uint32_t n_values, const navgpu_c3d_leaf* bounds,
                                        uint32_t n_bounds, int32_t* verdicts_out);

/* replaces: OctomapServerLayer3D::subscribe / subscribeUpdatesUnlocked (octomap_server_layer_3d.cpp:160-186) for one (instance,
 * layer) pair: the subscription state starts over (no full map seen, no update counted, updates not in use).  NAVGPU_ERR_STATE
 * before configure_layers; NAVGPU_ERR_INVALID for an instance or layer out of range or a cylinder layer. */
int navgpu_costmap3d_layer_resubscribe(navgpu_costmap3d* c3d, uint32_t instance, uint32_t layer);

#endif /* NAVGPU_COSTMAP3D_PUBLISH_H_ */
