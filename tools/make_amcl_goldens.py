#!/usr/bin/env python3
"""Write tests/golden/g9_amcl.npz from the reference amcl core itself (compiled in place, see tools/amcl_reference_build.py).

Seeded maps (free, occupied and unknown values; non-square; map_scale_up_factor 1 and 2) with the reference's
map_update_cspace distances, and per laser-model configuration one AMCLLaser::UpdateSensor per map: particles, a scan
(ray-cast from a true pose, with NaN and >= range_max beams), the resulting weights, w_slow / w_fast, `updated` and whether
LikelihoodFieldModelProb took its beam-skip error branch, with its per-beam obs_count where it skips beams.

Particles whose beam end point (or, for the beam model, ray-cast start / end cell) lies within 1e-7 cell of a cell boundary
are redrawn, so a device cell index equals the reference's despite <= 1-ulp libm differences.  The reference's single-thread
CPU time per update is printed (for DESIGN).  Usage: python tools/make_amcl_goldens.py [--out PATH]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import amcl_reference_build as B  # noqa: E402
import amcl_spec  # noqa: E402

ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "g9_amcl.npz")
MARGIN = 1e-7

# (msg width, msg height, resolution, scale_up_factor, origin, max_occ_dist)
MAPS = [(120, 90, 0.05, 1, (-3.0, -2.25), 0.5), (70, 50, 0.05, 2, (-1.5, -1.0), 0.4), (200, 150, 0.05, 1, (-5.0, -3.75), 2.0)]
LASER = (0.12, -0.03, 0.05)
RANGE_MAX = 4.0

BASE = dict(model_type=1, max_beams=30, z_hit=0.95, z_short=0.1, z_max=0.05, z_rand=0.05, sigma_hit=0.2, lambda_short=0.1, chi_outlier=0.0,
            do_beamskip=0, beam_skip_distance=0.5, beam_skip_threshold=0.3, beam_skip_error_threshold=0.9, gompertz_a=1.0,
            gompertz_b=1.0, gompertz_c=1.0, input_shift=0.0, input_scale=1.0, output_shift=0.0, off_map_factor=1.0,
            non_free_space_factor=1.0, non_free_space_radius=0.0, alpha_slow=0.001, alpha_fast=0.1)
# name -> (params, range_count, converged, w_slow / w_fast before)
CONFIGS = {
    "beam": (dict(model_type=0, max_beams=30), 181, 0, (0.0, 0.0)),
    "field": (dict(model_type=1, max_beams=30), 181, 0, (0.002, 0.004)),
    "field_factors": (dict(model_type=1, max_beams=60, off_map_factor=0.5, non_free_space_factor=0.25, non_free_space_radius=0.3),
                      1081, 0, (0.002, 0.004)),
    "beam_factors": (dict(model_type=0, max_beams=20, off_map_factor=0.7, non_free_space_factor=0.4, non_free_space_radius=0.25),
                     181, 0, (0.003, 0.001)),
    "prob": (dict(model_type=2, max_beams=30), 181, 0, (0.0, 0.0)),
    "prob_skip": (dict(model_type=2, max_beams=30, do_beamskip=1, beam_skip_distance=0.3, beam_skip_threshold=0.3,
                       beam_skip_error_threshold=0.9), 181, 1, (0.001, 0.002)),
    "prob_skip_unconverged": (dict(model_type=2, max_beams=30, do_beamskip=1, beam_skip_distance=0.3, beam_skip_threshold=0.3,
                                   beam_skip_error_threshold=0.9), 181, 0, (0.001, 0.002)),
    # every subsampled beam valid (range_count = 2 max_beams: step 2, no NaN / max range at even indices), so the
    # reference's error branch reads only entries it wrote in this update
    "prob_skip_error": (dict(model_type=2, max_beams=30, do_beamskip=1, beam_skip_distance=0.02, beam_skip_threshold=0.6,
                             beam_skip_error_threshold=0.2), 60, 1, (0.001, 0.002)),
    "gompertz": (dict(model_type=3, max_beams=30, gompertz_a=0.9, gompertz_b=3.0, gompertz_c=4.0, input_shift=-0.1, input_scale=1.5,
                      output_shift=0.05, z_rand=0.02), 181, 0, (0.001, 0.002)),
}


def make_map(rng, w, h):
    d = np.zeros((h, w), np.int8)
    d[0, :] = d[-1, :] = 100
    d[:, 0] = d[:, -1] = 100
    for _ in range(6):  # walls / boxes
        x0, y0 = rng.integers(2, w - 12), rng.integers(2, h - 12)
        ww, hh = rng.integers(1, 10), rng.integers(1, 10)
        d[y0:y0 + hh, x0:x0 + ww] = 100
    noise = rng.random((h, w))
    d[noise < 0.01] = 100
    d[(noise > 0.5) & (noise < 0.52)] = -1          # unknown
    d[(noise > 0.6) & (noise < 0.605)] = 50         # unknown (neither 0 nor 100)
    d[h // 3:h // 3 + 5, w - 12:w - 4] = -1         # an unknown block
    return d


def cell_frac(v, origin, scale):
    f = (v - origin) / scale + 0.5
    return np.abs(f - np.round(f))


def laser_poses(poses):
    a = np.asarray(LASER)
    c, s = np.cos(poses[:, 2]), np.sin(poses[:, 2])
    x = poses[:, 0] + a[0] * c - a[1] * s
    y = poses[:, 1] + a[0] * s + a[1] * c
    th = poses[:, 2] + a[2]
    return np.stack([x, y, np.arctan2(np.sin(th), np.cos(th))], 1)


def near_boundary(poses, ranges, origin, scale, beam_model):
    lp = laser_poses(poses)
    r = ranges[:, 0][None, :]
    ang = lp[:, 2:3] + ranges[:, 1][None, :]
    if beam_model:
        r = np.full_like(r, RANGE_MAX)
    ok = np.isfinite(r)
    hx = lp[:, 0:1] + np.where(ok, r, 0) * np.cos(ang)
    hy = lp[:, 1:2] + np.where(ok, r, 0) * np.sin(ang)
    bad = (cell_frac(hx, origin[0], scale) < MARGIN) | (cell_frac(hy, origin[1], scale) < MARGIN)
    bad = bad.any(1) | (cell_frac(lp[:, 0], origin[0], scale) < MARGIN) | (cell_frac(lp[:, 1], origin[1], scale) < MARGIN)
    return bad


def raycast_scan(rng, occ, origin, scale, pose, rc):
    sy, sx = occ.shape
    bearings = np.linspace(-np.pi / 2, np.pi / 2, rc)
    out = np.zeros((rc, 2))
    out[:, 1] = bearings
    for i, b in enumerate(bearings):
        a = pose[2] + b
        rr = RANGE_MAX
        for t in np.arange(0.0, RANGE_MAX, scale / 4):
            mi = int(np.floor((pose[0] + t * np.cos(a) - origin[0]) / scale + 0.5) + sx // 2)
            mj = int(np.floor((pose[1] + t * np.sin(a) - origin[1]) / scale + 0.5) + sy // 2)
            if not (0 <= mi < sx and 0 <= mj < sy) or occ[mj, mi] > -1:
                rr = t
                break
        out[i, 0] = min(RANGE_MAX, rr + rng.normal(0, 0.02)) if rr < RANGE_MAX else RANGE_MAX
    return out


def make_case(rng, occ, origin, scale, rc, spoil, beam_model, n):
    sy, sx = occ.shape
    free = np.argwhere(occ == -1)
    jy, jx = free[rng.integers(len(free))]
    true = np.array([origin[0] + (jx - sx // 2) * scale, origin[1] + (jy - sy // 2) * scale, rng.uniform(-np.pi, np.pi)])
    scan = raycast_scan(rng, occ, origin, scale, true, rc)
    if not spoil:
        scan[:, 0] = np.minimum(scan[:, 0], RANGE_MAX - 0.01)
    else:
        idx = rng.choice(rc, size=rc // 12, replace=False)
        scan[idx[: len(idx) // 2], 0] = np.nan
        scan[idx[len(idx) // 2:], 0] = RANGE_MAX + rng.choice([0.0, 0.5], size=len(idx) - len(idx) // 2)
    poses = np.zeros((n, 3))
    k = int(n * 0.8)
    poses[:k] = true + rng.normal(0, [0.08, 0.08, 0.04], size=(k, 3))
    span = np.array([sx * scale, sy * scale])
    lo = np.array(origin) - span / 2 - 0.3
    poses[k:, :2] = lo + rng.random((n - k, 2)) * (span + 0.6)   # some off the map, some on occupied / unknown cells
    poses[k:, 2] = rng.uniform(-np.pi, np.pi, n - k)
    while True:
        bad = near_boundary(poses, scan, origin, scale, beam_model)
        if not bad.any():
            break
        poses[bad] += rng.normal(0, 1e-3, size=(bad.sum(), 3))
    weights = rng.uniform(0.5, 1.5, n) / n
    return poses, weights, scan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if not B.available():
        sys.exit(f"the reference amcl tree is not at {B.AMCL}")
    rng = np.random.default_rng(1)
    G = {}
    with tempfile.TemporaryDirectory() as td:
        exe = B.build_harness(td)
        maps = []
        for m, (w, h, res, f, org, mod) in enumerate(MAPS):
            data = make_map(rng, w, h)
            occ = amcl_spec.convert_map(data, f)
            sy, sx = occ.shape
            scale = res / f
            centre = (org[0] + (sx // 2) * scale, org[1] + (sy // 2) * scale)  # AmclNode::convertMap
            t0 = time.perf_counter()
            dist = B.run_cspace(exe, td, occ, scale, mod)
            G[f"map{m}_data"], G[f"map{m}_dist"] = data, dist
            G[f"map{m}_geom"] = np.array([w, h, res, f, org[0], org[1], mod, centre[0], centre[1], scale])
            maps.append((occ, scale, centre, mod))
            print(f"map{m}: {sx}x{sy} R={int(mod / scale)}  map_update_cspace {1e3 * (time.perf_counter() - t0):.1f} ms (incl. process)")
        names = sorted(CONFIGS)
        G["configs"] = np.array(names)
        G["param_order"] = np.array(B.PARAM_ORDER)
        for name in names:
            over, rc, conv, w0 = CONFIGS[name]
            params = dict(BASE, **over)
            G[f"{name}_params"] = np.array([float(params[k]) for k in B.PARAM_ORDER])
            for m, (occ, scale, centre, mod) in enumerate(maps):
                n = 300 if m < 2 else 1000
                spoil = name != "prob_skip_error"
                poses, weights, scan = make_case(rng, occ, centre, scale, rc, spoil, params["model_type"] == 0, n)
                upd, ws, wf, wout, err, _, oc = B.run_update(exe, td, occ, scale, centre, mod, params, LASER, w0, conv, poses, weights, scan,
                                                      RANGE_MAX)
                key = f"{name}_m{m}"
                G[key + "_poses"], G[key + "_weights_in"], G[key + "_scan"] = poses, weights, scan
                G[key + "_state_in"] = np.array([w0[0], w0[1], conv, RANGE_MAX])
                G[key + "_out"] = np.concatenate([[upd, ws, wf, float(err)], wout])
                if oc is not None:
                    G[key + "_obs_count"] = oc
                print(f"{key}: updated={upd} error_branch={err} w_slow={ws:.6g} w_fast={wf:.6g}")
        # the reference's single-thread CPU time of one update: 5 000 particles x 30 beams, likelihood field, map2
        occ, scale, centre, mod = maps[2]
        poses, weights, scan = make_case(rng, occ, centre, scale, 181, True, False, 5000)
        for name in ("field", "beam", "prob"):
            params = dict(BASE, **CONFIGS[name][0])
            r = B.run_update(exe, td, occ, scale, centre, mod, params, LASER, (0, 0), 0, poses, weights, scan, RANGE_MAX)
            print(f"reference {name}: {r[5]:.3f} ms per AMCLLaser::UpdateSensor (5000 particles, 181 ranges, max_beams 30, one thread)")
    np.savez_compressed(args.out, **G)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
