#!/usr/bin/env python3
"""Write tests/golden/g18_global_planner_reference.npz: the cases of tests/global_planner_reference_cases.py and what the reference's
own global_planner classes make of them - DijkstraExpansion, AStarExpansion, PotentialCalculator, QuadraticCalculator, GradientPath and
GridPath (global_planner/src compiled in place, driven by tools/global_planner_reference_harness.cpp the way planner_core.cpp drives
them: setters through the Expander* / Traceback* members, calculatePotentials with nx * ny * 2 cycles, clearEndpoint, getPath).

dijkstra.h, astar.h and gradient_path.cpp include global_planner/planner_core.h, which needs ROS; the stand-in of
tools/global_planner_ref_stubs/ goes ahead of the reference's include directory and gives them the two things they want from it.
tools/navfn_ros_stubs/math.h goes ahead of everything: GradientPath's hypot on floats is C's hypot(double, double), as NavFn's is
(that header says why).  costmap_2d/cost_values.h is the reference's own.

  maps (+ map_index), shapes         the costmaps as a caller hands them over (before outlineMap), padded to the largest shape
  names, params, starts, goals, goal_cells     per plan; params columns are PARAM_KEYS, cost_factor apart in cost_factors
  found_legal                        calculatePotentials' return value
  potential_before, potential        the potential array before and after clearEndpoint (float32, padded like the maps)
  path_ret, path_len, path           getPath's return value (-1: not called), the number of points it left - also where it
                                     returned false - and the points, goal first, concatenated
  meta                               JSON: the reference files compiled, the flags, what is not recorded
The expansion's cycle count is a local of the reference and is not recorded.
Usage: python tools/make_global_planner_goldens.py [--out PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import global_planner_reference_cases as T  # noqa: E402

REFERENCE = os.environ.get("NAVGPU_REFERENCE", "/root/reference")
GP = os.path.join(REFERENCE, "global_planner")
OUT = T.GOLDEN
SOURCES = ("dijkstra.cpp", "astar.cpp", "gradient_path.cpp", "grid_path.cpp", "quadratic_calculator.cpp")
FLAGS = ("-std=c++14", "-O2", "-w", "-ffp-contract=off")


def available():
    return all(os.path.isfile(os.path.join(GP, "src", s)) for s in SOURCES) and \
        os.path.isfile(os.path.join(REFERENCE, "costmap_2d", "include", "costmap_2d", "cost_values.h"))


def build_harness(workdir):
    exe = os.path.join(workdir, "global_planner_reference_harness")
    subprocess.run(["g++", *FLAGS, "-I", os.path.join(HERE, "navfn_ros_stubs"), "-I", os.path.join(HERE, "global_planner_ref_stubs"),
                    "-I", os.path.join(ROOT, "tests", "ros_stubs"), "-I", os.path.join(GP, "include"),
                    "-I", os.path.join(REFERENCE, "costmap_2d", "include"), "-include", "algorithm", "-include", "cstring",
                    os.path.join(HERE, "global_planner_reference_harness.cpp")] + [os.path.join(GP, "src", s) for s in SOURCES] +
                   ["-o", exe, "-lm"], check=True)
    return exe


def run_harness(exe, workdir, plans):
    """plans: list of (cmap as calculatePotentials sees it, params dict, start_xy, goal_xy, goal_cell) ->
    list of dict(found_legal, potential_before, potential, path_ret, path)"""
    fin, fout = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(fin, "wb") as f:
        np.array([len(plans)], np.int64).tofile(f)
        for cm, p, s, g, gc in plans:
            ny, nx = cm.shape
            np.array([nx, ny, p["use_dijkstra"], p["use_quadratic"], p["use_grid_path"], p["old_navfn_behavior"], p["allow_unknown"],
                      p["lethal_cost"], p["neutral_cost"], gc[0], gc[1]], np.int32).tofile(f)
            np.array([p["cost_factor"], s[0], s[1], g[0], g[1]], np.float64).tofile(f)
            np.ascontiguousarray(cm, np.uint8).tofile(f)
    subprocess.run([exe, fin, fout], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    out, at = [], 0
    for cm, _, _, _, _ in plans:
        ny, nx = cm.shape
        ns = nx * ny
        legal = int(np.frombuffer(raw, np.int32, 1, at)[0])
        before = np.frombuffer(raw, np.float32, ns, at + 4).reshape(ny, nx).copy()
        after = np.frombuffer(raw, np.float32, ns, at + 4 + 4 * ns).reshape(ny, nx).copy()
        at += 4 + 8 * ns
        ret, n = (int(v) for v in np.frombuffer(raw, np.int32, 2, at))
        path = np.frombuffer(raw, np.float32, 2 * n, at + 8).reshape(n, 2).copy()
        at += 8 + 8 * n
        out.append(dict(found_legal=legal, potential_before=before, potential=after, path_ret=ret, path=path))
    assert at == len(raw)
    return out


def generate(workdir):
    exe = build_harness(workdir)
    cases = T.cases()
    res = run_harness(exe, workdir, [(T.outlined(c), T.full_params(c["params"]), c["start"], c["goal"], T.goal_cell(c)) for c in cases])
    maps, index = [], []
    for c in cases:
        for j, mp in enumerate(maps):
            if mp.shape == c["cmap"].shape and np.array_equal(mp, c["cmap"]):
                index.append(j)
                break
        else:
            index.append(len(maps))
            maps.append(c["cmap"])
    d = dict(maps=np.stack([T.pad(m, 0) for m in maps]), map_shapes=np.array([m.shape for m in maps], np.int32),
             map_index=np.array(index, np.int32), names=np.array([c["name"] for c in cases]),
             params=np.array([[T.full_params(c["params"])[k] for k in T.PARAM_KEYS] for c in cases], np.int32),
             cost_factors=np.array([T.full_params(c["params"])["cost_factor"] for c in cases], np.float64),
             starts=np.array([c["start"] for c in cases], np.float64), goals=np.array([c["goal"] for c in cases], np.float64),
             goal_cells=np.array([T.goal_cell(c) for c in cases], np.int32),
             found_legal=np.array([r["found_legal"] for r in res], np.int32),
             potential_before=np.stack([T.pad(r["potential_before"], 0.0) for r in res]),
             potential=np.stack([T.pad(r["potential"], 0.0) for r in res]),
             path_ret=np.array([r["path_ret"] for r in res], np.int32), path_len=np.array([len(r["path"]) for r in res], np.int32),
             path=np.concatenate([r["path"] for r in res]).astype(np.float32))
    d["meta"] = np.array(json.dumps(dict(
        sources=["global_planner/src/" + s for s in SOURCES], flags=list(FLAGS), math_h="tools/navfn_ros_stubs/math.h (the C header)",
        param_keys=list(T.PARAM_KEYS), driven_as="planner_core.cpp: setters through Expander* / Traceback*",
        not_recorded="the expansion's cycle count (a local of calculatePotentials)", n_cases=len(cases))))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if not available():
        print("the reference global_planner tree is not on this machine: nothing written")
        return
    with tempfile.TemporaryDirectory() as wd:
        d = generate(wd)
    np.savez_compressed(a.out, **d)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, {len(d['names'])} plans")


if __name__ == "__main__":
    main()
