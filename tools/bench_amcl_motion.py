#!/usr/bin/env python3
"""Time navgpu_amcl_update_action (AMCLOdom::UpdateAction) for 256 filters x {500, 5 000} particles, every model, in drand48 mode
(the reference's stream, regenerated on the device) and with device draws (Philox).  Host wall time per call, which ends in a
stream synchronise and the state download, median of --steps.  Then the full cycle motion -> sensor -> resample with the set
resident on the device, against the path without a device motion model: get_samples, the motion on the host (numpy, the same
model with numpy's generator), set_samples, then the same sensor update and resample.  Prints one JSON line.  The reference's
single-thread time per call is printed by tools/make_amcl_motion_goldens.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import navigation_amd as nav  # noqa: E402

MODELS = ("diff", "omni", "diff_corrected", "omni_corrected", "gaussian")


def host_motion(P, counts, odom, alphas, rng):
    """numpy stand-in for the host's motion step (diff-corrected, amcl_odom.cpp:276-320) with numpy's generator"""
    a1, a2, a3, a4 = alphas[:4]
    for f in range(len(P)):
        n = int(counts[f])
        d = odom[f, 3:6]
        dt = np.hypot(d[0], d[1])
        r1 = np.arctan2(d[1], d[0]) - (odom[f, 2] - d[2])
        r2 = d[2] - r1
        z = rng.standard_normal((n, 3))
        r1h = r1 - np.sqrt(a1 * r1 * r1 + a2 * dt * dt) * z[:, 0]
        th = dt - np.sqrt(a3 * dt * dt + a4 * r1 * r1 + a4 * r2 * r2) * z[:, 1]
        r2h = r2 - np.sqrt(a1 * r2 * r2 + a2 * dt * dt) * z[:, 2]
        p = P[f, :n]
        p[:, 0] += th * np.cos(p[:, 2] + r1h)
        p[:, 1] += th * np.sin(p[:, 2] + r1h)
        p[:, 2] += r1h + r2h


def med_ms(ts):
    return round(1e3 * float(np.median(ts)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="500,5000")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    nF = args.filters
    out = {"filters": nF, "timing": "host wall per call incl. synchronise, median"}
    occ = np.zeros((2000, 2000), np.int8)
    occ[rng.random(occ.shape) < 0.01] = 100
    bearings = np.linspace(-2.0, 2.0, 360)
    scans = [np.stack([rng.uniform(0.5, 8.0, 360), bearings], 1) for _ in range(nF)]
    for n in (int(s) for s in args.sizes.split(",")):
        a = nav.AmclLaser(nF, n, 30)
        P = np.zeros((nF, n, 3))
        P[..., 0] = rng.uniform(-45, 45, (nF, 1)) + rng.normal(0, 0.5, (nF, n))
        P[..., 1] = rng.uniform(-45, 45, (nF, 1)) + rng.normal(0, 0.5, (nF, n))
        P[..., 2] = rng.uniform(-3, 3, (nF, 1)) + rng.normal(0, 0.3, (nF, n))
        W = np.full((nF, n), 1.0 / n)
        odom = np.column_stack([rng.normal(0, 5, (nF, 3)), rng.normal(0, 0.1, (nF, 3)), np.abs(rng.normal(0, 0.1, (nF, 3)))])
        a.set_samples(P, W)
        for model, name in enumerate(MODELS):
            a.configure_odom(model, 0.2, 0.2, 0.2, 0.2, 0.2)
            for mode in ("drand48", "device"):
                state = np.array([nav.localization.drand48_state(k) for k in range(nF)], np.uint64)
                ts = []
                for i in range(args.warmup + args.steps):
                    t0 = time.perf_counter()
                    if mode == "drand48":
                        _, _, state = a.update_action(odom, drand48_state=state)
                    else:
                        a.update_action(odom, seed=i)
                    if i >= args.warmup:
                        ts.append(time.perf_counter() - t0)
                out[f"{name}_{mode}_{n}_ms"] = med_ms(ts)
        # the full cycle, resident and with the host motion step
        a.set_map(occ, 0.05, (-50.0, -50.0), max_occ_dist=2.0)
        a.configure(model_type=1, max_beams=30)
        a.configure_resample(resample_model=0, min_samples=100)
        a.configure_odom(2, 0.2, 0.2, 0.2, 0.2, 0.2)
        hrng = np.random.default_rng(1)
        for path in ("resident", "host_motion"):
            a.set_samples(P, W)
            a.set_filter_state(np.tile([[1.0, 1.0]], (nF, 1)))
            state = np.array([nav.localization.drand48_state(k) for k in range(nF)], np.uint64)
            ts, parts = [], {"motion": [], "sensor": [], "resample": []}
            for i in range(args.warmup + args.steps):
                t0 = time.perf_counter()
                if path == "resident":
                    _, _, state = a.update_action(odom, drand48_state=state)
                else:
                    sc, Ph, Wh, cv = a.get_samples()
                    host_motion(Ph, sc, odom, (0.2, 0.2, 0.2, 0.2), hrng)
                    a.set_samples(Ph, Wh, sample_counts=sc, converged=cv)
                t1 = time.perf_counter()
                a.update_sensor(scans, 10.0)
                t2 = time.perf_counter()
                a.update_resample(seed=i)
                t3 = time.perf_counter()
                if i >= args.warmup:
                    ts.append(t3 - t0)
                    parts["motion"].append(t1 - t0)
                    parts["sensor"].append(t2 - t1)
                    parts["resample"].append(t3 - t2)
            out[f"cycle_{path}_{n}_ms"] = med_ms(ts)
            for k, v in parts.items():
                out[f"cycle_{path}_{n}_{k}_ms"] = med_ms(v)
        a.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
