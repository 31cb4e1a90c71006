#!/usr/bin/env python3
"""Time one navgpu_amcl_node_laser_received call for 256 filters x {500, 5 000} particles against the same work through the step
entry points, as a caller had to do it before: the scan converted on the host, update_action / update_sensor / update_resample
split into runs of the filters that are due, one navgpu_amcl_get_clusters per publishing filter.

Two cases: every robot updating, and one robot in four.  Scans of 360 rays, max_beams 30, likelihood field, resample_interval 1
(so a filter that is due runs motion, sensor, resample and the read-out), one shared 2000 x 2000 map.  Both paths are driven
through the C entry points with buffers marshalled beforehand, start every step from the same re-uploaded sets (outside the
timed region), use the same seed and alternate within each step; their sets are compared byte for byte once.  Host wall time
around calls that end in a stream wait.

--baseline-lib PATH takes the step entry points from another build of libnavgpu.so (the parent commit's), in the same process.
The spread is the difference between the medians of the even and the odd steps of the same path.  Prints one JSON line (ms)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import navigation_amd as nav  # noqa: E402
from navigation_amd import _lib  # noqa: E402
from navigation_amd import localization  # noqa: E402

RAYS, MAX_BEAMS = 360, 30


def load_baseline(path):
    L = C.CDLL(path)
    for name, res, args in _lib.SYMBOLS:
        if hasattr(L, name):  # a parent build has no navgpu_amcl_node_*
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    return L


def make(L, nF, n, occ, res):
    saved = localization.lib
    localization.lib = lambda: L
    try:
        a = nav.AmclLaser(nF, n, MAX_BEAMS)
    finally:
        localization.lib = saved
    a.set_map(occ, res, (-50.0, -50.0), max_occ_dist=2.0)
    a.configure(max_beams=MAX_BEAMS)
    a.set_laser_pose(np.tile([0.1, 0.0, 0.0], (nF, 1)))
    a.configure_odom(_lib.AMCL_ODOM_DIFF)
    a.configure_resample(min_samples=100)
    return a


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--samples", type=int, nargs="*", default=[500, 5000])
    ap.add_argument("--baseline-lib", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    nF, res = args.filters, 0.05
    occ = np.zeros((2000, 2000), np.int8)
    occ[rng.random(occ.shape) < 0.01] = 100
    L = nav.lib()
    LB = load_baseline(args.baseline_lib) if args.baseline_lib else L
    out = {"filters": nF, "rays": RAYS, "baseline": "other build" if args.baseline_lib else "same build"}
    raw = rng.uniform(0.5, 8.0, (nF, RAYS)).astype(np.float32)
    raw[:, ::17] = 0.01  # some short readings
    yaw_min, yaw_inc, rmin, rmax = -1.57, -1.57 + 3.14 / (RAYS - 1), np.float32(0.1), np.float32(10.0)
    for n in args.samples:
        a, b = make(L, nF, n, occ, res), make(LB, nF, n, occ, res)
        a.configure_node(d_thresh=0.2, a_thresh=0.5, resample_interval=1)
        P = np.zeros((nF, n, 3))
        centre = np.stack([rng.uniform(-45, 45, nF), rng.uniform(-45, 45, nF), rng.uniform(-3, 3, nF)], 1)
        P[..., 0] = centre[:, :1] + rng.normal(0, 0.5, (nF, n))
        P[..., 1] = centre[:, 1:2] + rng.normal(0, 0.5, (nF, n))
        P[..., 2] = centre[:, 2:] + rng.normal(0, 0.3, (nF, n))
        W = np.full((nF, n), 1.0 / n)
        for case, stride in (("all", 1), ("quarter", 4)):
            due = np.arange(nF) % stride == 0
            pose0 = np.zeros((nF, 3))
            pose1 = pose0 + np.where(due[:, None], [0.3, 0.0, 0.05], 0.0)
            state = a.node_state()
            state.pf_init[:] = 1
            state.lasers_update[:] = 0
            state.force_update[:] = 0
            state.latest_tf_valid[:] = 1
            state.pf_odom_pose[:] = pose0
            # path A: the records of the one call
            scans = (_lib.AmclScan * nF)()
            for f in range(nF):
                s = scans[f]
                s.flags, s.range_count, s.range_offset, s.range_min, s.range_max = 1, RAYS, f * RAYS, rmin, rmax
                s.yaw_min, s.yaw_inc, s.odom_pose = yaw_min, yaw_inc, tuple(pose1[f])
            results = np.zeros(nF, localization.NODE_RESULT_DTYPE)
            # path B: buffers of the step calls
            odom = np.concatenate([pose1, pose1 - pose0, np.zeros((nF, 3))], 1)
            counts = np.full(nF, RAYS, np.uint32)
            rmaxd = np.full(nF, float(rmax))
            st, upd, ncl = np.zeros(nF, np.int32), np.zeros(nF, np.int32), C.c_int32()
            cw, cm, sc9 = np.zeros(n), np.zeros((n, 3)), np.zeros(9)
            idx = np.arange(RAYS, dtype=np.float64)
            inc = np.fmod(yaw_inc - yaw_min + 5 * np.pi, 2 * np.pi) - np.pi
            runs = [(0, nF)] if stride == 1 else [(int(f), 1) for f in np.nonzero(due)[0]]
            hyp = np.zeros((nF, 3))

            def by_hand(seed):
                beams = np.empty((nF, RAYS, 2))  # amcl_node.cpp:1524-1537 on the host
                beams[..., 0] = np.where(raw <= rmin, rmax, raw)
                beams[..., 1] = yaw_min + idx * inc
                for first, cnt in runs:
                    LB.navgpu_amcl_update_action(b.h, first, cnt, p(odom[first:]), _lib.AMCL_DRAW_DEVICE, None, seed, p(st))
                    LB.navgpu_amcl_update_sensor(b.h, first, cnt, p(beams[first:]), p(counts), p(rmaxd), p(upd))
                    LB.navgpu_amcl_update_resample(b.h, first, cnt, _lib.AMCL_DRAW_DEVICE, None, None, None, None, seed, p(st))
                    for f in range(first, first + cnt):
                        LB.navgpu_amcl_get_clusters(b.h, f, C.byref(ncl), n, None, p(cw), p(cm), None, None, p(sc9))
                        hyp[f] = cm[int(np.argmax(cw[:ncl.value]))]

            ta, tb = [], []
            for i in range(args.warmup + args.steps):
                for h in (a, b):
                    h.set_samples(P, W)
                    h.set_rng_counters(np.zeros(nF, np.uint64))
                a.set_node_state(state)
                order = (0, 1) if i % 2 == 0 else (1, 0)
                for which in order:
                    t0 = time.perf_counter()
                    if which == 0:
                        rc = L.navgpu_amcl_node_laser_received(a.h, 0, nF, C.byref(scans), p(raw), i, p(results))
                    else:
                        by_hand(i)
                    t = time.perf_counter() - t0
                    if i >= args.warmup:
                        (ta if which == 0 else tb).append(t)
                assert rc == 0, rc
                if i == 0:  # the same work: the same bytes
                    r = results.view(np.recarray)
                    assert r.resampled.tolist() == due.astype(int).tolist() and r.published.tolist() == due.astype(int).tolist()
                    assert np.array_equal(r.pose[due], hyp[due])
                    sa, sb = a.get_samples(), b.get_samples()
                    assert all(np.array_equal(x, y) for x, y in zip(sa, sb)), "the two paths' sets differ"
            ta, tb = 1e3 * np.array(ta), 1e3 * np.array(tb)
            key = f"{case}_{n}"
            out[f"{key}_node_ms"] = round(float(np.median(ta)), 3)
            out[f"{key}_steps_ms"] = round(float(np.median(tb)), 3)
            out[f"{key}_node_spread_ms"] = round(abs(float(np.median(ta[0::2]) - np.median(ta[1::2]))), 3)
            out[f"{key}_steps_spread_ms"] = round(abs(float(np.median(tb[0::2]) - np.median(tb[1::2]))), 3)
            out[f"{key}_node_p10_p90_ms"] = [round(float(v), 3) for v in np.percentile(ta, [10, 90])]
            out[f"{key}_steps_p10_p90_ms"] = [round(float(v), 3) for v in np.percentile(tb, [10, 90])]
        a.close()
        b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
