#!/usr/bin/env python3
"""Time navgpu_amcl_update_sensor (amcl's laser sensor update) for 256 filters x {500, 5 000} particles x 30 beams per model on
one shared 2000 x 2000 map, and navgpu_amcl_set_map (conversion + exact distance transform) for 2000^2 and 4000^2 maps.
Prints one JSON line (ms, host wall time per call including the scan upload and the final synchronisation)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import navigation_amd as nav  # noqa: E402


def world(n, rng):
    d = np.zeros((n, n), np.int8)
    d[rng.random((n, n)) < 0.002] = 100
    for _ in range(n // 20):  # walls
        x, y = rng.integers(0, n - 200, 2)
        if rng.random() < 0.5:
            d[y, x:x + 200] = 100
        else:
            d[y:y + 200, x] = 100
    d[rng.random((n, n)) < 0.01] = -1
    return d


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    res, nF = 0.05, args.filters
    out = {"filters": nF, "beams": 30, "range_count": 181}
    a = nav.AmclLaser(nF, 5000, 30)
    for n in (2000, 4000):
        data = world(n, rng)
        t = timed(lambda: a.set_map(data, res, (-n * res / 2, -n * res / 2), max_occ_dist=2.0), max(3, args.steps // 4), 1)
        out[f"distance_map_{n}_ms"] = round(t, 3)
    data = world(2000, rng)
    a.set_map(data, res, (-50.0, -50.0), max_occ_dist=2.0)
    scans = []
    for k in range(nF):
        s = np.zeros((181, 2))
        s[:, 0] = rng.uniform(0.3, 9.0, 181)
        s[:, 1] = np.linspace(-np.pi / 2, np.pi / 2, 181)
        s[rng.random(181) < 0.03, 0] = 10.0
        scans.append(s)
    a.set_laser_pose(np.tile([0.1, 0.0, 0.0], (nF, 1)))
    for n in (500, 5000):
        P = np.zeros((nF, n, 3))
        P[..., 0] = rng.uniform(-45, 45, (nF, 1)) + rng.normal(0, 0.3, (nF, n))
        P[..., 1] = rng.uniform(-45, 45, (nF, 1)) + rng.normal(0, 0.3, (nF, n))
        P[..., 2] = rng.uniform(-3, 3, (nF, n))
        W = np.full((nF, n), 1.0 / n)
        for name, kw in (("beam", dict(model_type=0)), ("field", dict(model_type=1)), ("prob", dict(model_type=2)),
                         ("prob_beamskip", dict(model_type=2, do_beamskip=1)), ("gompertz", dict(model_type=3))):
            a.configure(max_beams=30, **kw)
            a.set_samples(P, W, converged=np.ones(nF))

            def step():
                a.update_sensor(scans, 10.0)
            out[f"{name}_{n}_ms"] = round(timed(step, args.steps, args.warmup), 3)
    a.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
