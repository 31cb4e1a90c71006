"""numpy statements of what the amcl device path is specified to compute (used by the goldens generator and the tests).

exact_cspace: the exact capped Euclidean distance transform of navgpu_amcl_set_map (include/navgpu.h).
convert_map:  AmclNode::convertMap's occupancy conversion (amcl_node.cpp:1062-1093).
"""
import numpy as np


def convert_map(data, scale_up_factor=1):
    """OccupancyGrid data (height, width) int8 -> map_t occ_state (height * f, width * f): 0 -> -1, 100 -> +1, else 0."""
    d = np.asarray(data, np.int8)
    occ = np.where(d == 0, -1, np.where(d == 100, 1, 0)).astype(np.int8)
    f = int(scale_up_factor)
    return np.repeat(np.repeat(occ, f, axis=0), f, axis=1)


def exact_cspace(occ_state, scale, max_occ_dist):
    """D = smallest dx^2 + dy^2 to an occupied cell; (float)(sqrt(D) * scale) if sqrt(D) <= (int)(max_occ_dist / scale), else
    (float)max_occ_dist.  Separable: nearest occupied cell per column, then the minimum of dx^2 + g^2 along the row."""
    occ = np.asarray(occ_state) == 1
    sy, sx = occ.shape
    R = int(max_occ_dist / scale)
    big = np.int64(1) << 40
    ys = np.arange(sy, dtype=np.int64)[:, None]
    last = np.maximum.accumulate(np.where(occ, ys, -big), axis=0)
    nxt = np.minimum.accumulate(np.where(occ, ys, 2 * big)[::-1], axis=0)[::-1]
    g = np.minimum(ys - last, nxt - ys)
    g2 = np.where(g <= R, g * g, big)
    D = g2.copy()
    for dx in range(1, min(R, sx) + 1):
        D[:, dx:] = np.minimum(D[:, dx:], g2[:, :-dx] + dx * dx)
        D[:, :-dx] = np.minimum(D[:, :-dx], g2[:, dx:] + dx * dx)
    out = np.full((sy, sx), np.float32(max_occ_dist), np.float32)
    inside = D <= R * R
    out[inside] = (np.sqrt(D[inside].astype(np.float64)) * scale).astype(np.float32)
    return out


def brute_cspace(occ_state, scale, max_occ_dist):
    """The same by brute force over every occupied cell (small maps only)."""
    occ = np.asarray(occ_state) == 1
    sy, sx = occ.shape
    R = int(max_occ_dist / scale)
    oy, ox = np.nonzero(occ)
    out = np.full((sy, sx), np.float32(max_occ_dist), np.float32)
    if len(oy) == 0:
        return out
    yy, xx = np.mgrid[0:sy, 0:sx]
    D = np.full((sy, sx), np.int64(1) << 40)
    for y, x in zip(oy, ox):
        D = np.minimum(D, (yy - y) ** 2 + (xx - x) ** 2)
    inside = D <= R * R
    out[inside] = (np.sqrt(D[inside].astype(np.float64)) * scale).astype(np.float32)
    return out
