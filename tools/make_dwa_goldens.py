#!/usr/bin/env python3
"""Write tests/golden/g15_dwa_reference.npz: DWA planning cycles as the reference's own classes compute them.

tools/dwa_reference_harness.cpp compiles dwa_local_planner::DWAPlanner, LocalPlannerUtil, goal_functions, SimpleTrajectoryGenerator,
the four critic classes, SimpleScoredSamplingPlanner, MapGrid, CostmapModel and Costmap2D in place (NAVGPU_REFERENCE, against
tools/dwa_ref_stubs/ and tests/ros_stubs/) and runs the cases below.  The file holds inputs and reference outputs only: neither the
CPU oracle nor the library is imported here (the maps are inflated by the few numpy lines of inflate()).

Per case NAME (see tests/dwa_reference_cases.py for the decoder):
  NAME_in     the harness's input doubles: mode, sizes, configuration, footprint, per-cycle pose / velocity / plan, checkTrajectory samples
  NAME_map    index into map_K (uint8 costmaps)
  NAME_cyc    per cycle: pos[3], vel[3], critic scale[6], n_slots, winner {found, slot, xv, yv, thetav, cost, n_points}, drive[3],
              oscillation flags, prev_stationary_pos[3]
  NAME_slot   per slot of every cycle: sample[3], accepted, n_points, trajectory velocities[3], raw critic[6] (oscillation, obstacle,
              goal_front, alignment, path, goal), total without early-out, total in all_explored
  NAME_traj   the winners' points, concatenated
  NAME_grid   per cycle the path, goal and goal_front MapGrid distances (uint16; every value is a cell count <= size + 1)
  NAME_check  DWAPlanner::checkTrajectory's answers after the last cycle
meta (JSON): wiring per case, compile flags, and which rollout_trig mode equals the reference's trajectory points on this toolchain.
Usage: python tools/make_dwa_goldens.py [--out PATH]
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
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dwa_reference_cases as D  # noqa: E402

REFERENCE = os.environ.get("NAVGPU_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "g15_dwa_reference.npz")
FLAGS = ["-std=c++14", "-O2", "-w", "-ffp-contract=off"]
BLP = ["simple_trajectory_generator", "obstacle_cost_function", "map_grid_cost_function", "map_grid", "map_cell", "oscillation_cost_function",
       "simple_scored_sampling_planner", "costmap_model", "footprint_helper", "trajectory", "local_planner_util", "goal_functions",
       "map_grid_visualizer"]
COSTMAP = ["costmap_2d", "costmap_math", "footprint", "array_parser"]


def sources():
    return ([os.path.join(REFERENCE, "base_local_planner", "src", s + ".cpp") for s in BLP] +
            [os.path.join(REFERENCE, "costmap_2d", "src", s + ".cpp") for s in COSTMAP] +
            [os.path.join(REFERENCE, "dwa_local_planner", "src", "dwa_planner.cpp")])


def available():
    return all(os.path.isfile(s) for s in sources())


def build_harness(workdir):
    exe = os.path.join(workdir, "dwa_reference_harness")
    inc = [os.path.join(HERE, "dwa_ref_stubs"), os.path.join(ROOT, "tests", "ros_stubs")] + [
        os.path.join(REFERENCE, p, "include") for p in ("base_local_planner", "costmap_2d", "dwa_local_planner", "nav_core")]
    cmd = ["g++"] + FLAGS + [a for i in inc for a in ("-I", i)] + [os.path.join(HERE, "dwa_reference_harness.cpp")] + sources() + [
        "-o", exe, "-lpthread", "-lm"]
    subprocess.run(cmd, check=True)
    return exe


def run_harness(exe, workdir, cases, maps):
    fin, fout = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(fin, "wb") as f:
        np.array([len(cases)], np.int64).tofile(f)
        for c in cases:
            d = D.encode_input(c, maps[c["map"]].shape)
            np.array([len(d)], np.int64).tofile(f)
            d.tofile(f)
            m = np.ascontiguousarray(maps[c["map"]], np.uint8)
            np.array([m.size], np.int64).tofile(f)
            m.tofile(f)
        probe = D.trig_probe()
        np.array([len(probe)], np.int64).tofile(f)
        probe.tofile(f)
    subprocess.run([exe, fin, fout], check=True)
    raw = np.fromfile(fout, np.uint8)
    out, at = [], 0
    for _ in cases:
        n = int(raw[at:at + 8].view(np.int64)[0])
        out.append(raw[at + 8:at + 8 + 8 * n].view(np.float64).copy())
        at += 8 + 8 * n
    probe_out = raw[at:].view(np.float64).reshape(-1, 3).copy()
    assert len(probe_out) == len(probe)
    return out, probe, probe_out


def generate(workdir):
    cases, maps = D.build_cases()
    exe = build_harness(workdir)
    outs, probe, probe_out = run_harness(exe, workdir, cases, maps)
    d = {f"map_{i}": m for i, m in enumerate(maps)}
    for c, o in zip(cases, outs):
        name = c["name"]
        shape = maps[c["map"]].shape
        rec = D.decode_output(o, c, shape)
        d[name + "_in"] = D.encode_input(c, shape)
        d[name + "_map"] = np.array(c["map"], np.int32)
        for k in ("cyc", "slot", "traj", "grid", "check"):
            d[f"{name}_{k}"] = rec[k]
        # the poses the reference derived through tf are the float32 inputs
        for k, cyc in enumerate(c["cycles"]):
            assert np.array_equal(rec["cyc"][k, 0:3].astype(np.float32), np.asarray(cyc["pos"], np.float32)), name
            assert np.array_equal(rec["cyc"][k, 3:6].astype(np.float32), np.asarray(cyc["vel"], np.float32)), name
    d["trig_probe_in"], d["trig_probe_out"] = probe.astype(np.float32), probe_out.astype(np.float32)
    trig, differ = D.trig_mode(probe, probe_out)
    meta = dict(
        rollout_trig=int(trig), rollout_trig_probe_states_that_tell_the_modes_apart=differ,
        flags=" ".join(FLAGS),
        compiled_in_place=[os.path.relpath(s, REFERENCE) for s in sources()],
        wiring={c["name"]: ("DWAPlanner" if c["mode"] == 0 else "direct") for c in cases},
        direct_wiring_restates="dwa_planner.cpp:57-81,116-127,167-179,240-286,298-319,357-368,217-230; every DWAPlanner case is also run "
                               "through it and compared double for double",
        sets={c["name"]: c["set"] for c in cases},
        fleet={c["name"]: dict(max_sim_steps=c.get("max_sim_steps", 128)) for c in cases},
        cases=[c["name"] for c in cases])
    d["meta"] = np.array(json.dumps(meta, sort_keys=True))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference base_local_planner / dwa_local_planner / costmap_2d trees are not on this machine")
    with tempfile.TemporaryDirectory() as wd:
        d = generate(wd)
    np.savez_compressed(a.out, **d)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, {len(d)} arrays")


if __name__ == "__main__":
    main()
