"""The yardstick of the costmap_3d queries: pure numpy in float64, independent of the library.

What a query computes is geometry: a triangle mesh at a pose against the closed cubes of the occupied cells.  Every (cell, triangle)
pair is looked at with the definitions the header states:
  overlap    the 13-axis separating-axis test of a triangle against a cube (closed sets: touching overlaps)
  interior   closed mesh only: the winding number of a cell's centre from the triangles' solid angles, |w| > 0.5
  distance   the minimum over the closest feature pairs of two disjoint convex polytopes: 3 vertex-cube, 8 corner-triangle and
             36 edge-edge distances
  regions    RegionsOfInterestAtPose's half-spaces at the pose; a cell is out when centre distance - extent > 0 for one of them
  fold       Costmap3DROS::processPlanCost3D's
Brute force over the (cell, triangle) pairs, less those two bounds rule out - bounds, not heuristics: the answers are those over
all pairs.  A cube more than a whole cell away from the posed mesh's bounding box touches no triangle and holds no interior
point, so the overlap and interior tests skip it.  A cube further from that box than the smallest vertex-cube distance (an upper
bound of the answer that is cheap and exact) cannot hold the minimum, so the feature distances skip it."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max
DBL_MIN = np.finfo(np.float64).tiny
COST, COLLISION_ONLY, DISTANCE = 0, 1, 2
ALL, LEFT, RIGHT, RECTANGULAR_PRISM = 0, 1, 2, 3


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def rotation(q):
    """the rotation matrix of a quaternion (x, y, z, w), normalised first"""
    x, y, z, w = np.asarray(q, np.float64) / np.sqrt(np.sum(np.square(np.asarray(q, np.float64))))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def yaw_pose(x, y, th):
    return np.array([x, y, 0.0, 0.0, 0.0, np.sin(th * 0.5), np.cos(th * 0.5)])


def pad_points(vertices, padding):
    """Costmap3DQuery::padPoints: every vertex pushed radially in xy, in float; the origin left alone"""
    v = np.array(vertices, np.float64)
    if padding == 0.0:
        return v
    for i in range(len(v)):
        x, y, pad = np.float32(v[i, 0]), np.float32(v[i, 1]), np.float32(padding)
        dist = np.float32(np.sqrt(np.float32(x * x + y * y)))
        if dist == 0:
            continue
        v[i, 0] = np.float32(np.float32(x / dist) * np.float32(dist + pad))
        v[i, 1] = np.float32(np.float32(y / dist) * np.float32(dist + pad))
    return v


def mesh_closed(triangles):
    """every directed edge has its opposite exactly once"""
    edges = {}
    for t in np.asarray(triangles).reshape(-1, 3):
        for k in range(3):
            e = (int(t[k]), int(t[(k + 1) % 3]))
            edges[e] = edges.get(e, 0) + 1
    return all(n == 1 and edges.get((b, a), 0) == 1 for (a, b), n in edges.items())


def mesh_volume(vertices, triangles):
    p = np.asarray(vertices, np.float64)[np.asarray(triangles).reshape(-1, 3)]
    return float(np.sum(_dot(p[:, 0], _cross(p[:, 1], p[:, 2]))) / 6.0)


def world_triangles(vertices, triangles, pose):
    R, T = rotation(pose[3:7]), np.asarray(pose[:3], np.float64)
    w = np.asarray(vertices, np.float64) @ R.T + T
    return w[np.asarray(triangles).reshape(-1, 3)]  # (nt, 3, 3)


def region_mask(centres, size, region, scale, pose):
    """checkROI per cell: True where the cell is considered"""
    keep = np.ones(len(centres), bool)
    if region == ALL:
        return keep
    if region == LEFT:
        planes = [((0.0, -1.0, 0.0), 0.0)]
    elif region == RIGHT:
        planes = [((0.0, 1.0, 0.0), 0.0)]
    else:
        planes = [((-1.0, 0.0, 0.0), 0.0), ((0.0, 1.0, 0.0), scale[1] / 2.0), ((0.0, -1.0, 0.0), scale[1] / 2.0),
                  ((0.0, 0.0, 1.0), scale[2] / 2.0), ((0.0, 0.0, -1.0), scale[2] / 2.0)]
    R, T = rotation(pose[3:7]), np.asarray(pose[:3], np.float64)
    for n, d in planes:
        n = R @ np.array(n)
        d = d + n @ T
        extent = 0.5 * np.sum(np.abs(n * size))
        keep &= ~(centres @ n - d > extent)
    return keep


def overlap(V, h):
    """V: (N, nt, 3, 3) triangles relative to N cube centres, h the cubes' half edge -> (N, nt) bool"""
    e = [V[:, :, 1] - V[:, :, 0], V[:, :, 2] - V[:, :, 1], V[:, :, 0] - V[:, :, 2]]
    unit = np.eye(3)
    axes = [np.broadcast_to(unit[i], e[0].shape) for i in range(3)] + [_cross(e[0], e[1])]
    axes += [_cross(e[i], np.broadcast_to(unit[j], e[0].shape)) for i in range(3) for j in range(3)]
    hit = np.ones(V.shape[:2], bool)
    for a in axes:
        p = np.stack([_dot(a, V[:, :, k]) for k in range(3)], -1)
        r = h * (np.abs(a[..., 0]) + np.abs(a[..., 1]) + np.abs(a[..., 2]))
        hit &= ~((p.min(-1) > r) | (p.max(-1) < -r))
    return hit


def winding(centres, tris):
    """(N,) winding numbers of the points about the mesh (van Oosterom and Strackee's solid angle per triangle)"""
    V = tris[None] - centres[:, None, None, :]
    a, b, c = V[:, :, 0], V[:, :, 1], V[:, :, 2]
    la, lb, lc = (np.sqrt(_dot(v, v)) for v in (a, b, c))
    num = _dot(a, _cross(b, c))
    den = la * lb * lc + _dot(a, b) * lc + _dot(a, c) * lb + _dot(b, c) * la
    return np.sum(2.0 * np.arctan2(num, den), -1) / (4.0 * np.pi)


def _point_segment2(p, a, ab):
    t = np.clip(_dot(p - a, ab) / _dot(ab, ab), 0.0, 1.0)
    d = p - (a + ab * t[..., None])
    return _dot(d, d)


def _segment_segment2(p1, d1, p2, d2):
    r = p1 - p2
    a, e, f, c, b = _dot(d1, d1), _dot(d2, d2), _dot(d2, r), _dot(d1, r), _dot(d1, d2)
    denom = a * e - b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(denom != 0.0, np.clip((b * f - c * e) / denom, 0.0, 1.0), 0.0)
    t = (b * s + f) / e
    s = np.where(t < 0.0, np.clip(-c / a, 0.0, 1.0), np.where(t > 1.0, np.clip((b - c) / a, 0.0, 1.0), s))
    t = np.clip(t, 0.0, 1.0)
    d = (p1 + d1 * s[..., None]) - (p2 + d2 * t[..., None])
    return _dot(d, d)


def distance2(V, h):
    """V as in overlap, the triangles disjoint from the cubes -> (N, nt) squared distances"""
    q = np.maximum(np.abs(V) - h, 0.0)
    best = np.min(_dot(q, q), -1)
    v = [V[:, :, 0], V[:, :, 1], V[:, :, 2]]
    e = [v[1] - v[0], v[2] - v[1], v[0] - v[2]]
    n = _cross(e[0], e[1])
    nn = _dot(n, n)
    for k in range(8):
        c = np.broadcast_to(np.array([h if k & 1 else -h, h if k & 2 else -h, h if k & 4 else -h]), v[0].shape)
        inside = np.ones(V.shape[:2], bool)
        for i in range(3):
            inside &= _dot(_cross(e[i], c - v[i]), n) >= 0.0
        plane = np.square(_dot(c - v[0], n)) / nn
        edges = np.minimum(np.minimum(_point_segment2(c, v[0], e[0]), _point_segment2(c, v[1], e[1])), _point_segment2(c, v[2], e[2]))
        best = np.minimum(best, np.where(inside, plane, edges))
    w = 2.0 * h
    for axis in range(3):
        d2 = np.zeros(3)
        d2[axis] = w
        for k in range(4):
            u, s = (h if k & 1 else -h), (h if k & 2 else -h)
            p2 = np.array([[-h, u, s], [u, -h, s], [u, s, -h]][axis])
            for i in range(3):
                best = np.minimum(best, _segment_segment2(v[i], e[i], np.broadcast_to(p2, v[i].shape), np.broadcast_to(d2, v[i].shape)))
    return best


def query_pose(centres, size, vertices, triangles, pose, mode=DISTANCE, region=ALL, scale=(0.0, 0.0, 0.0), limit=DBL_MAX, closed=None,
               half_scale=1.0):
    """One pose against the occupied cells `centres` (N, 3) of edge `size`.  Returns the pose's cost as the header defines it.
    half_scale scales the cubes' half edge in the overlap test (the decided-pose check of the golden poses)."""
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    closed = mesh_closed(triangles) if closed is None else closed
    tris = world_triangles(vertices, triangles, pose)
    centres = centres[region_mask(centres, size, region, scale, pose)]
    h = 0.5 * size
    if limit <= 0.0:
        limit = DBL_MIN
    if len(centres) == 0:
        return limit if mode == DISTANCE else 0.0
    # a cube more than a cell away from the posed mesh's bounding box touches no triangle and holds no interior point
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    gap = np.maximum(np.maximum(lo - (centres + h), (centres - h) - hi), 0.0)
    close = centres[(gap <= size).all(1)]
    if len(close):
        if overlap(tris[None] - close[:, None, None, :], h * half_scale).any():
            return -1.0
        if closed and (np.abs(winding(close, tris)) > 0.5).any():
            return -1.0
    if mode != DISTANCE:
        return 0.0
    # the pairs that can hold the minimum (see the module's docstring)
    V = tris[None] - centres[:, None, None, :]
    q = np.maximum(np.abs(V) - h, 0.0)
    upper2 = np.min(_dot(q, q))
    near = _dot(gap, gap) <= upper2 * (1.0 + 1e-9)  # (the two are rounded differently)
    d = float(np.sqrt(np.min(distance2(V[near], h))))
    return d if d < limit else limit


def fold(pose_costs, mode, lazy=False):
    """processPlanCost3D's fold over one run -> dict(cost, n_lethal, first_lethal, n_done)"""
    cost = DBL_MAX if mode == DISTANCE else 0.0
    n_lethal, first, n_done = 0, -1, len(pose_costs)
    for j, pc in enumerate(pose_costs):
        collision = pc < 0.0
        if mode == DISTANCE:
            cost = min(cost, pc)
        elif collision:
            cost = pc if cost >= 0.0 else cost + pc
        elif cost >= 0.0:
            cost += pc
        if collision:
            n_lethal += 1
            first = j if first < 0 else first
            if lazy:
                n_done = j + 1
                break
    return dict(cost=cost, n_lethal=n_lethal, first_lethal=first, n_done=n_done)


def cell_centres(cells, origin, size):
    """the centres of the cells (N, 3) integer indices of a grid, as the library places them"""
    return np.asarray(origin, np.float64) + (np.asarray(cells, np.float64).reshape(-1, 3) + 0.5) * size


CUBE_VERTICES = np.array([[x, y, z] for z in (0.0, 1.0) for y in (0.0, 1.0) for x in (0.0, 1.0)])
# the unit cube [0, 1]^3: 12 triangles, outward normals
CUBE_TRIANGLES = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                           [1, 3, 5], [3, 7, 5]], np.uint32)
TETRA_VERTICES = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
TETRA_TRIANGLES = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.uint32)


def boxes_to_cells(centres, sizes, origin, size):
    """octomap leaves of any depth as the integer indices (N, 3) of their finest cells in the grid at `origin` with edge `size`"""
    out = []
    centres, sizes = np.asarray(centres, np.float64).reshape(-1, 3), np.broadcast_to(np.asarray(sizes, np.float64), (len(centres),))
    for c, s in zip(centres, sizes):
        n = int(round(s / size))
        first = np.rint((c - 0.5 * s - np.asarray(origin)) / size).astype(np.int64)
        g = np.arange(n)
        out.append(first + np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    return np.concatenate(out) if out else np.zeros((0, 3), np.int64)
