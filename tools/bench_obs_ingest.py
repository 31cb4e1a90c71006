#!/usr/bin/env python3
"""What handing a costmap cycle its sensor data costs, two ways, for the contract fleet (256 robots, 400 x 400 cells, one
720-beam LaserScan per robot and cycle):
  stage : today's hand-over - the host holds every kept observation in the global frame, height-filtered, and
          navgpu_costmap_stage uploads all of them every cycle - then navgpu_costmap_update;
  obsbuf: navgpu_obsbuf_buffer with the cycle's new scan as ranges in the sensor's frame, navgpu_obsbuf_stage, then
          navgpu_costmap_update: the kept clouds stay on the device.
Each with observation_keep_time = 0 (one observation per robot) and with a keep time that keeps 4 scans.  Everything a cycle
hands over is marshalled before the timed loops (ctypes arrays and packed numpy buffers); the stage path's points are the very
points the obsbuf path computes (read back once with navgpu_obsbuf_observations), so the two fleets run the same cycles - the
tool checks that their master grids end up equal.  A cycle's time is the host clock from the first call to a drained stream.
The two paths run alternately in blocks (A/B/A/B...); reported are the median and the spread of the block medians, and the
host-to-device bytes per cycle of both, computed from the shapes.  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_FORCE_BLIT_COPY_SIZE", "2048")  # as bench.py: small host-to-device copies through the copy kernels

BEAMS, SCANS, S = 720, 8, 1_000_000_000
PERIOD = S // 10  # a scan every 0.1 s


def align256(v):
    return (v + 255) & ~255


def make_fleet(nav, n, cells, kept):
    from navigation_amd import _lib as N, synth
    fl = nav.Fleet(n, cells, cells, synth.RES, layers=N.LAYER_OBSTACLE | N.LAYER_INFLATION, max_points=BEAMS * kept, max_observations=kept)
    fl.configure_obstacle()
    fl.set_footprint(synth.FOOTPRINT)
    fl.configure_inflation(synth.INFLATION_RADIUS, synth.COST_SCALING, synth.inscribed_radius(synth.FOOTPRINT))
    return fl


def scan_ranges(rs, n):
    """n x BEAMS float32: walls 1 - 2.4 m away that differ from robot to robot, a few beams without a return"""
    i = np.arange(BEAMS)
    r = 1.7 + 0.6 * np.sin(i[None, :] / 40.0 + rs.uniform(0, 6.28, (n, 1))) + rs.normal(0, 0.01, (n, BEAMS))
    r[rs.uniform(size=r.shape) < 0.02] = np.inf
    return np.ascontiguousarray(r, np.float32)


class Run:
    """the two fleets of one keep-time setting, with everything their cycles hand over"""

    def __init__(self, nav, n, cells, kept, seed):
        from navigation_amd import _lib as N, synth
        self.n, self.kept, self.N = n, kept, N
        rs = np.random.RandomState(seed)
        half = cells * synth.RES / 2
        self.poses = np.ascontiguousarray(np.stack([half + rs.uniform(-0.5, 0.5, n), half + rs.uniform(-0.5, 0.5, n), rs.uniform(-3, 3, n)], 1))
        src = [dict(observation_keep_time_ns=(kept - 1) * PERIOD, inf_is_valid=1)]
        self.A, self.B = make_fleet(nav, n, cells, kept), make_fleet(nav, n, cells, kept)
        self.B.obs_configure(src, slots=kept, max_cloud_points=BEAMS)
        # the obsbuf path's hand-over: SCANS pre-built cloud arrays (the stamp is patched per cycle) and their ranges
        self.no_points = np.zeros((0, 3), np.float32)
        self.clouds = []
        for c in range(SCANS):
            r = scan_ranges(rs, n)
            arr, _, rng = self.B.pack_clouds([dict(instance=i, stamp_ns=0, ranges=r[i], angle_min=-math.pi, angle_increment=2 * math.pi / BEAMS,
                                                   range_min=0.1, range_max=3.0, origin=(self.poses[i, 0], self.poses[i, 1], 0.3),
                                                   transform=[math.cos(self.poses[i, 2]), -math.sin(self.poses[i, 2]), 0, math.sin(self.poses[i, 2]),
                                                              math.cos(self.poses[i, 2]), 0, 0, 0, 1, self.poses[i, 0], self.poses[i, 1], 0.3])
                                              for i in range(n)])
            self.clouds.append((arr, rng, np.frombuffer(arr, dtype=np.dtype(N.Cloud))["stamp_ns"]))
        # the stage path's hand-over: the same scans as the device projects, transforms and filters them, read back once on a
        # scratch fleet, then per cycle the `kept` newest of them, newest first, as one packed Observation array
        scratch = make_fleet(nav, n, 64, 1)
        scratch.obs_configure([dict(observation_keep_time_ns=0, inf_is_valid=1)], slots=1, max_cloud_points=BEAMS)
        per_scan = []
        for c in range(SCANS):
            arr, rng, _ = self.clouds[c]
            scratch.obs_buffer_raw(arr, n, self.no_points, rng, 0)
            per_scan.append([scratch.obs_observations(i)[0]["points"] for i in range(n)])
        scratch.close()
        for j in range(kept - 1, 0, -1):  # the scans "before cycle 0", so that cycle 0 already finds kept - 1 older ones
            arr, rng, stamps = self.clouds[-j % SCANS]
            stamps[:] = -j * PERIOD
            self.B.obs_buffer_raw(arr, n, self.no_points, rng, -j * PERIOD)
        self.staged = []
        for c in range(SCANS):
            arr = (N.Observation * (n * kept))()
            pts, off, k = [], 0, 0
            for i in range(n):
                for j in range(kept):
                    p = per_scan[(c - j) % SCANS][i]
                    arr[k] = N.Observation(i, off, len(p), N.OBS_MARKING | N.OBS_CLEARING, self.poses[i, 0], self.poses[i, 1], 0.3, 2.5, 3.0)
                    pts.append(p)
                    off += len(p)
                    k += 1
            self.staged.append((arr, np.ascontiguousarray(np.concatenate(pts), np.float32)))
        mo, mp = kept, BEAMS * kept
        common = align256(24 * n) + align256(512 * n) + align256(4 * n) + align256(56 * n * mo) + align256(4 * n)
        self.h2d_stage = common + align256(12 * n * mp)  # the whole staging block: navgpu_costmap_stage copies it as one
        self.h2d_obsbuf = (24 + 512 + 4 + 56 * mo + 4) * n + align256(104 * n) + align256(4 * BEAMS * n)
        self.h2d_stage_points = int(np.mean([s[1].nbytes for s in self.staged]))

    def cycle_stage(self, k):
        arr, pts = self.staged[k % SCANS]
        self.A.stage_observations_raw(self.poses, arr, self.n * self.kept, pts)
        self.A.update_map()
        self.A.sync()

    def cycle_obsbuf(self, k):
        arr, rng, stamps = self.clouds[k % SCANS]
        now = k * PERIOD
        stamps[:] = now
        self.B.obs_buffer_raw(arr, self.n, self.no_points, rng, now)
        self.B.obs_stage(self.poses, now, want_current=False)
        self.B.update_map()
        self.B.sync()

    def block(self, fn, k0, steps):
        t = []
        for k in range(k0, k0 + steps):
            t0 = time.perf_counter()
            fn(k)
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t))

    def measure(self, warmup, steps, blocks):
        k = 0
        for fn in (self.cycle_stage, self.cycle_obsbuf):
            self.block(fn, 0, warmup)
        k = warmup
        a, b = [], []
        for _ in range(blocks):
            a.append(self.block(self.cycle_stage, k, steps))
            b.append(self.block(self.cycle_obsbuf, k, steps))
            k += steps
        equal = self.A.master().tobytes() == self.B.master().tobytes()
        marked = int((self.B.download(self.N.GRID_OBSTACLE) == 254).sum())
        out = dict(kept=self.kept, stage_ms=float(np.median(a)), stage_ms_min_max=[min(a), max(a)], obsbuf_ms=float(np.median(b)),
                   obsbuf_ms_min_max=[min(b), max(b)], h2d_bytes_stage=self.h2d_stage, h2d_bytes_stage_points_used=self.h2d_stage_points,
                   h2d_bytes_obsbuf=self.h2d_obsbuf, grids_equal=bool(equal), lethal_cells=marked)
        self.A.close()
        self.B.close()
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=256)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--steps", type=int, default=200, help="cycles per block")
    ap.add_argument("--blocks", type=int, default=5, help="A/B blocks of each path")
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import navigation_amd as nav
    if nav.lib().navgpu_device_count() <= 0:
        raise SystemExit("bench_obs_ingest: no HIP device (there is no CPU fallback, and a CPU timing would say nothing)")
    res = [Run(nav, args.robots, args.size, kept, 11 + kept).measure(args.warmup, args.steps, args.blocks) for kept in (1, 4)]
    print(json.dumps(dict(tool="bench_obs_ingest", robots=args.robots, size=args.size, beams=BEAMS, steps=args.steps, blocks=args.blocks,
                          cycle="hand-over + navgpu_costmap_update to a drained stream, host clock, median of block medians (ms)", runs=res)))


if __name__ == "__main__":
    main()
