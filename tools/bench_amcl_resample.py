#!/usr/bin/env python3
"""Time navgpu_amcl_update_resample (pf_update_resample + histogram + pf_cluster_stats + pf_update_converged) with device draws for
256 filters x {500, 5 000} particles, multinomial and systematic, on one shared 2000 x 2000 map.  Each call starts from the same
sensor-weighted set (set_samples and set_filter_state are re-uploaded outside the timed region).  Prints one JSON line (ms, host
wall time per call including the status download, median of --steps).  The reference's single-thread time per call is printed
by tools/make_amcl_resample_goldens.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import navigation_amd as nav  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    nF, res = args.filters, 0.05
    occ = np.zeros((2000, 2000), np.int8)
    occ[rng.random(occ.shape) < 0.01] = 100
    out = {"filters": nF, "draws": "device"}
    for n in (500, 5000):
        a = nav.AmclLaser(nF, n, 30)
        a.set_map(occ, res, (-50.0, -50.0), max_occ_dist=2.0)
        P = np.zeros((nF, n, 3))
        P[..., 0] = rng.uniform(-45, 45, (nF, 1)) + rng.normal(0, 0.5, (nF, n))  # one hypothesis per filter, some spread
        P[..., 1] = rng.uniform(-45, 45, (nF, 1)) + rng.normal(0, 0.5, (nF, n))
        P[..., 2] = rng.uniform(-3, 3, (nF, 1)) + rng.normal(0, 0.3, (nF, n))
        W = rng.uniform(0.2, 1.0, (nF, n))
        W /= W.sum(1, keepdims=True)
        for name, model in (("multinomial", 0), ("systematic", 1)):
            a.configure_resample(resample_model=model, min_samples=100)
            ts, counts = [], []
            for i in range(args.warmup + args.steps):
                a.set_samples(P, W)
                a.set_filter_state(np.tile([[1.0, 0.9]], (nF, 1)))  # w_diff = 0.1: random poses from the free cells too
                t0 = time.perf_counter()
                a.update_resample(seed=i)
                t = time.perf_counter() - t0
                if i >= args.warmup:
                    ts.append(t)
                    counts.append(float(np.mean(a.get_samples()[0])))
            out[f"{name}_{n}_ms"] = round(1e3 * float(np.median(ts)), 3)
            out[f"{name}_{n}_mean_count"] = round(float(np.mean(counts)), 1)
        a.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
