#!/usr/bin/env python3
"""Write tests/golden/g14_navfn_ros.npz: the navfn_ros tests' inputs (tests/navfn_ros_ref.py: batch_cases, the weight cases, the
serpentine) and what the reference's own navfn::NavFn (navfn/src/navfn.cpp compiled in place, driven by tools/navfn_ros_harness.cpp
as NavfnROS::makePlan drives it) makes of them: the potential array after calcNavFnDijkstra(true) and, from the best cell of the
tolerance window over that array, the path calcPath(nx * 4) finds in the same NavFn object - gradients memoised by the expansion's
own calcPath included.

Per case set S (batch, weights, serpentine):
  S_maps (+ S_map_index), S_frames, S_starts, S_goals, S_tolerances, S_weights     the inputs
  S_status, S_found, S_best_cell, S_best_xy, S_best_cost, S_candidates   per plan (best_cell -1 without one)
  S_potential                                             the reference's potarr per plan attempted (float32), S_attempted says which
  S_path, S_path_len                                      the second paths, concatenated, and their lengths (getPathLen())
  S_path_ret                                              calcPath's return value: 0 where the walk failed.  The reference's
                                                          getPlanFromPotential does not look at it and makes a plan of the S_path_len
                                                          points walked so far; the library (and S_status) report NO_PLAN there
navfn.h's <math.h> is the C header (tools/navfn_ros_stubs/math.h says why): NavFn's hypot on floats is hypot(double, double).
The window search between the two harness runs is tests/navfn_ros_ref.py's; tests/test_navfn_ros_reference.py checks it against a
literal transcription of the reference's loops.
Usage: python tools/make_navfn_ros_goldens.py [--out PATH]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import navfn_ros_ref as R  # noqa: E402

REFERENCE = os.environ.get("NAVGPU_REFERENCE", "/root/reference")
NAVFN = os.path.join(REFERENCE, "navfn")
OUT = os.path.join(ROOT, "tests", "golden", "g14_navfn_ros.npz")
WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (1.0, 0.01)]
SETS = ("batch", "weights", "serpentine")


def available():
    return os.path.isfile(os.path.join(NAVFN, "src", "navfn.cpp"))


def case_set(name):
    """-> list of (cmap, frame, start, goal, tolerance, w_dist, w_len)"""
    if name == "batch":
        return [c + (1.0, 0.0) for c in R.batch_cases()[0]]
    if name == "weights":
        return [R.blocked_goal_case() + (0.3,) + w for w in WEIGHTS] + [R.ring_case() + w for w in WEIGHTS]
    return [R.serpentine_case() + (0.0, 1.0, 0.0)]


def build_harness(workdir):
    exe = os.path.join(workdir, "navfn_ros_harness")
    subprocess.run(["g++", "-O2", "-w", "-ffp-contract=off", "-I", os.path.join(HERE, "navfn_ros_stubs"), "-I", os.path.join(ROOT, "tests", "ros_stubs"),
                    "-I", os.path.join(NAVFN, "include"),
                    "-include", "algorithm", "-include", "cstring", os.path.join(HERE, "navfn_ros_harness.cpp"),
                    os.path.join(NAVFN, "src", "navfn.cpp"), "-o", exe, "-lm"], check=True)
    return exe


def run_harness(exe, workdir, jobs):
    """jobs: list of (cmap, robot_cell, goal_cell, best_cell or None) -> list of (found, potarr (ny, nx), path (n, 2), calcPath's return value)"""
    fin, fout = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(fin, "wb") as f:
        np.array([len(jobs)], np.int64).tofile(f)
        for cm, robot, goal, best in jobs:
            ny, nx = cm.shape
            np.array([nx, ny, 1, robot[0], robot[1], goal[0], goal[1]] + list(best if best is not None else (-1, -1)), np.int32).tofile(f)
            np.ascontiguousarray(cm, np.uint8).tofile(f)
    subprocess.run([exe, fin, fout], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    out, at = [], 0
    for cm, _, _, _ in jobs:
        ny, nx = cm.shape
        found = int(np.frombuffer(raw, np.int32, 1, at)[0])
        pot = np.frombuffer(raw, np.float32, nx * ny, at + 4).reshape(ny, nx).copy()
        at += 4 + 4 * nx * ny
        ret, n = (int(v) for v in np.frombuffer(raw, np.int32, 2, at))
        path = np.frombuffer(raw, np.float32, 2 * n, at + 8).reshape(n, 2).copy()
        at += 8 + 8 * n
        out.append((found, pot, path, ret))
    assert at == len(raw)
    return out


def generate(workdir):
    exe = build_harness(workdir)
    d = {}
    for name in SETS:
        cases = case_set(name)
        maps, index = [], []
        for c in cases:
            for j, mp in enumerate(maps):
                if np.array_equal(mp, c[0]):
                    index.append(j)
                    break
            else:
                index.append(len(maps))
                maps.append(c[0])
        d[name + "_maps"] = np.stack(maps)
        d[name + "_map_index"] = np.array(index, np.int32)
        d[name + "_frames"] = np.array([c[1] for c in cases], np.float64)
        d[name + "_starts"] = np.array([c[2] for c in cases], np.float64)
        d[name + "_goals"] = np.array([c[3] for c in cases], np.float64)
        d[name + "_tolerances"] = np.array([c[4] for c in cases], np.float64)
        d[name + "_weights"] = np.array([c[5:7] for c in cases], np.float64)
        # makePlan's cells and early statuses; then the reference's expansion, the window over ITS array, and its second path
        pre = [R.make_plan(None, c[0], c[1], c[2], c[3], c[4], potential=np.full(c[0].shape, R.POT_HIGH, np.float32)) for c in cases]
        attempted = [k for k, p in enumerate(pre) if p["goal_cell"] is not None]
        first = run_harness(exe, workdir, [(cases[k][0], pre[k]["start_cell"], pre[k]["goal_cell"], None) for k in attempted])
        searches = [R.window_search(pot, cases[k][1], cases[k][3], cases[k][4], cases[k][5], cases[k][6]) for k, (_, pot, _, _) in zip(attempted, first)]
        second = run_harness(exe, workdir, [(cases[k][0], pre[k]["start_cell"], pre[k]["goal_cell"], b["cell"] if b else None)
                                            for k, (_, b) in zip(attempted, searches)])
        n = len(cases)
        status = np.array([p["status"] for p in pre], np.int32)
        found, cand = np.zeros(n, np.int32), np.zeros(n, np.int32)
        best_cell, best_xy, best_cost = np.full((n, 2), -1, np.int32), np.zeros((n, 2)), np.zeros(n)
        path_len, path_ret = np.zeros(n, np.int32), np.zeros(n, np.int32)
        paths = []
        for k, (f1, pot1, _, _), (c_, b), (f2, pot2, path, ret) in zip(attempted, first, searches, second):
            assert f1 == f2 and pot1.tobytes() == pot2.tobytes()
            found[k], cand[k] = f1, c_
            if b:
                best_cell[k], best_xy[k], best_cost[k] = b["cell"], (b["x"], b["y"]), b["cost"]
            assert ret in (0, len(path))
            path_len[k], path_ret[k] = len(path), ret
            paths.append(path)
            status[k] = R.OK if ret else R.NO_PLAN
        d[name + "_attempted"] = np.array(attempted, np.int32)
        d[name + "_status"], d[name + "_found"], d[name + "_candidates"] = status, found, cand
        d[name + "_best_cell"], d[name + "_best_xy"], d[name + "_best_cost"] = best_cell, best_xy, best_cost
        d[name + "_potential"] = np.stack([pot for _, pot, _, _ in first])
        d[name + "_path"] = np.concatenate(paths).astype(np.float32)
        d[name + "_path_len"], d[name + "_path_ret"] = path_len, path_ret
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if not available():
        print("the reference navfn tree is not on this machine: nothing written")
        return
    with tempfile.TemporaryDirectory() as wd:
        d = generate(wd)
    np.savez_compressed(a.out, **d)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
