#!/usr/bin/env python3
"""Time navgpu_amcl_init_gaussian / navgpu_amcl_init_uniform (pf_init / pf_init_model with uniformPoseGenerator) for 256 filters x
{500, 5 000} particles in drand48 mode (the reference's stream, regenerated on the device) and with device draws: the Gaussian,
the unscored uniform, and the scored uniform with the likelihood-field and beam models (threshold and multiplier chosen so that
retries happen).  Host wall time per call, which ends in a stream synchronise and the filter-table download, median of --steps;
the mean candidates per sample of the scored calls.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import navigation_amd as nav  # noqa: E402


def world():
    occ = -np.ones((200, 240), np.int8)
    occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = 1
    occ[60:140, 100:108] = 1
    occ[150:156, 20:180] = 1
    return occ, 0.05, (0.0, 0.0)


def scan(occ, scale, org, pose, n=180):
    """ranges to the nearest occupied cell along each bearing from `pose` (a synthetic scan of the map)"""
    sy, sx = occ.shape
    b = np.linspace(-math.pi / 2, math.pi / 2, n)
    r = np.full(n, 8.0)
    for k, bb in enumerate(b):
        for d in np.arange(0.05, 8.0, 0.025):
            i = int(math.floor((pose[0] + d * math.cos(pose[2] + bb) - org[0]) / scale + 0.5) + sx // 2)
            j = int(math.floor((pose[1] + d * math.sin(pose[2] + bb) - org[1]) / scale + 0.5) + sy // 2)
            if not (0 <= i < sx and 0 <= j < sy) or occ[j, i] == 1:
                r[k] = d
                break
    return np.stack([r, b], 1)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nf = a.filters
    occ, scale, org = world()
    s = scan(occ, scale, org, (-1.0, 1.5, 0.4))
    scans = [s] * nf
    res = {"filters": nf, "timing": "host wall per call incl. synchronise, median"}
    for ms in (500, 5000):
        h = nav.AmclLaser(nf, ms, max_beams=60)
        h.set_map_cells(occ, scale, org, max_occ_dist=2.0)
        h.set_laser_pose(np.tile([0.1, 0.0, 0.0], (nf, 1)))
        states = np.arange(1, nf + 1, dtype=np.uint64) << np.uint64(16) | np.uint64(0x330E)
        cov = np.diag([0.25, 0.25, 0.07])
        for src in ("drand48", "device"):
            kw = dict(drand48_state=states) if src == "drand48" else dict(seed=5)
            res[f"gaussian_{src}_{ms}_ms"], _ = timed(lambda: h.init_gaussian([0.0, 0.0, 0.0], cov, **kw), a.steps, a.warmup)
            res[f"uniform_{src}_{ms}_ms"], _ = timed(lambda: h.init_uniform(**kw), a.steps, a.warmup)
            for name, model, thr, mult in (("lf", 1, 3.0, 0.9), ("beam", 0, 1.5, 0.9)):
                h.configure(model_type=model, max_beams=60, z_hit=0.5, z_rand=0.5, sigma_hit=0.2)
                ms_, out = timed(lambda: h.init_uniform(scans, 8.0, threshold=thr, deweight_multiplier=mult, **kw),
                                 max(1, a.steps // 4), 1)
                res[f"uniform_scored_{name}_{src}_{ms}_ms"] = ms_
                res[f"uniform_scored_{name}_{src}_{ms}_candidates_per_sample"] = float(out[3].mean()) / ms
        h.close()
    res = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
