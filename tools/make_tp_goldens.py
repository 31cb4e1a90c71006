#!/usr/bin/env python3
"""Write tests/golden/g16_tp_reference.npz: legacy TrajectoryPlanner cycles as the reference's own class computes them.

tools/tp_reference_harness.cpp compiles base_local_planner::TrajectoryPlanner, CostmapModel, MapGrid, MapCell, FootprintHelper,
Trajectory, Costmap2D and costmap_2d's footprint.cpp in place (NAVGPU_REFERENCE, against tools/tp_ref_stubs/, tools/dwa_ref_stubs/
and tests/ros_stubs/) and runs the cases of tests/tp_reference_cases.py.  The file holds inputs and reference outputs only: neither
the CPU oracle nor the library is imported here.

Per case NAME (see tests/tp_reference_cases.py for the decoder):
  NAME_in      the harness's input doubles: sizes, origin, configuration, footprint, per cycle reconfigure / plan / pose / probes
  NAME_map     index into map_K (uint8 costmaps)
  NAME_cyc     per cycle: the configuration read back from the planner object (37), pos[3], vel[3] (the Eigen::Vector3f), n_pre,
               n_calls, winner {xv, yv, thetav, cost, n_points, call index}, drive[3], flags, prev_x, prev_y, escape_x, escape_y,
               escape_theta, n_within, n_post
  NAME_call    every generateTrajectory call of every cycle in call order: vx, vy, vtheta, cost_, points, last point[3]
  NAME_traj    the returned trajectories' points, concatenated
  NAME_within  the within_robot cells of every cycle (y * size_x + x), concatenated
  NAME_grid    per cycle the path_map_ and goal_map_ distances (uint16; every value is a cell count <= size + 1)
  NAME_pre     scoreTrajectory before findBestPath (after updatePlan), NAME_post  scoreTrajectory, checkTrajectory after it
meta (JSON): compile flags, the sources compiled in place, the fleet capacity per case, the knife-edge margin measured.
Usage: python tools/make_tp_goldens.py [--out PATH] [--show]
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
import tp_reference_cases as T  # noqa: E402

REFERENCE = os.environ.get("NAVGPU_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "g16_tp_reference.npz")
FLAGS = ["-std=c++14", "-O2", "-w", "-ffp-contract=off"]
WRAP = "-Wl,--wrap=_ZN18base_local_planner10Trajectory11resetPointsEv"  # base_local_planner::Trajectory::resetPoints()
BLP = ["trajectory_planner", "costmap_model", "map_grid", "map_cell", "footprint_helper", "trajectory"]
COSTMAP = ["costmap_2d", "footprint", "costmap_math", "array_parser"]
# One ulp at 1000 cells is about 1e-13 cells; over at most 128 accumulated steps that is about 1e-11; the guard allows 100 times that.
# A case closer than this to a cell boundary is moved by its author (the generator fails), never dropped.
KNIFE_EDGE = 1e-9


def sources():
    return ([os.path.join(REFERENCE, "base_local_planner", "src", s + ".cpp") for s in BLP] +
            [os.path.join(REFERENCE, "costmap_2d", "src", s + ".cpp") for s in COSTMAP])


def available():
    return all(os.path.isfile(s) for s in sources())


def build_harness(workdir):
    exe = os.path.join(workdir, "tp_reference_harness")
    inc = [os.path.join(HERE, "tp_ref_stubs"), os.path.join(HERE, "dwa_ref_stubs"), os.path.join(ROOT, "tests", "ros_stubs")] + [
        os.path.join(REFERENCE, p, "include") for p in ("base_local_planner", "costmap_2d", "nav_core")]
    cmd = ["g++"] + FLAGS + [a for i in inc for a in ("-I", i)] + [os.path.join(HERE, "tp_reference_harness.cpp")] + sources() + [
        WRAP, "-o", exe, "-lpthread", "-lm"]
    subprocess.run(cmd, check=True)
    return exe


def run_harness(exe, workdir, cases, maps):
    fin, fout = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(fin, "wb") as f:
        np.array([len(cases)], np.int64).tofile(f)
        for c in cases:
            d = T.encode_input(c, maps[c["map"]].shape)
            np.array([len(d)], np.int64).tofile(f)
            d.tofile(f)
            m = np.ascontiguousarray(maps[c["map"]], np.uint8)
            np.array([m.size], np.int64).tofile(f)
            m.tofile(f)
    subprocess.run([exe, fin, fout], check=True)
    raw = np.fromfile(fout, np.uint8)
    out, at = [], 0
    for _ in cases:
        n = int(raw[at:at + 8].view(np.int64)[0])
        out.append(raw[at + 8:at + 8 + 8 * n].view(np.float64).copy())
        at += 8 + 8 * n
    assert at == len(raw)
    return out


def generate(workdir):
    cases, maps = T.build_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    for m in maps:
        assert not (m == T.NOINFO).any(), "no NO_INFORMATION cells: the reference's rule for them is an uninitialised read"
        assert 64 <= min(m.shape) and max(m.shape) <= 160
    exe = build_harness(workdir)
    outs = run_harness(exe, workdir, cases, maps)
    # every case again with the other allow_unknown (the other Costmap2D default value): without unknown cells the two must agree in
    # every recorded double (the last one, allow_unknown_ as the planner read it, is an uninitialised read and is not compared)
    others = run_harness(exe, workdir, [dict(c, allow_unknown=1 - c["allow_unknown"]) for c in cases], maps)
    for c, a, b in zip(cases, outs, others):
        assert np.array_equal(a[:-1], b[:-1], equal_nan=True), f"{c['name']}: allow_unknown 0 and 1 differ on a map without unknown cells"
    unique, index = [], []
    for m in maps:  # cases that share a map share its array
        for i, u in enumerate(unique):
            if u.shape == m.shape and np.array_equal(u, m):
                index.append(i)
                break
        else:
            unique.append(m)
            index.append(len(unique) - 1)
    d = {f"map_{i}": m for i, m in enumerate(unique)}
    margins = {}
    for c, o in zip(cases, outs):
        name = c["name"]
        shape = maps[c["map"]].shape
        rec, margins[name] = T.decode_output(o, c, shape)
        assert margins[name] >= KNIFE_EDGE, f"{name}: a rollout point or footprint vertex lies {margins[name]:.3e} cells from a cell boundary"
        d[name + "_in"] = T.encode_input(c, shape)
        d[name + "_map"] = np.array(index[c["map"]], np.int32)
        for k in ("cyc", "call", "traj", "within", "grid", "pre", "post"):
            d[f"{name}_{k}"] = rec[k]
        for k, cyc in enumerate(T.unpack(c, rec)):
            if c["cycles"][k]["mode"] == 0:  # the floats handed in are the floats the planner used
                assert np.array_equal(cyc.pos, c["cycles"][k]["pos"]) and np.array_equal(cyc.vel, c["cycles"][k]["vel"]), name
            for call in cyc.calls:  # every trajectory starts at the pose the planner derived
                assert call[4] <= c["max_sim_steps"], name
            if cyc.n_points:
                assert np.array_equal(cyc.traj[0], cyc.pos.astype(np.float64)), name
    meta = dict(
        flags=" ".join(FLAGS + [WRAP]),
        compiled_in_place=[os.path.relpath(s, REFERENCE) for s in sources()],
        calls_observed="Trajectory::resetPoints() wrapped at link time names the object a generateTrajectory call fills; the unlock of "
                       "configuration_mutex_ (the harness's boost::mutex stand-in) marks the call's end",
        knife_edge_bound_cells=KNIFE_EDGE, knife_edge_margin_cells=margins, knife_edge_min_cells=min(margins.values()),
        allow_unknown_both_values_agree=len(cases),
        fleet={c["name"]: dict(max_sim_steps=c["max_sim_steps"]) for c in cases},
        cases=[c["name"] for c in cases])
    d["meta"] = np.array(json.dumps(meta, sort_keys=True))
    return d, cases


def show(d, cases):
    """One line per cycle: what won and what state it left (for the author of a case)."""
    meta = json.loads(str(d["meta"]))
    names = "SL SR RL RR SLS SRS StL StR ESC".split()
    for c in cases:
        _, _, cycles = T.case(d, meta, c["name"])
        print(f"{c['name']}  margin {meta['knife_edge_margin_cells'][c['name']]:.2e}")
        for k, cy in enumerate(cycles):
            st = cy.stage_of(cy.best_call)
            legal = {s: sum(cy.calls[i][3] >= 0 for i in cy.stage_calls(s)) for s in range(5)}
            codes = sorted({float(x) for x in cy.calls[:, 3] if x < 0})
            fl = "|".join(n for b, n in enumerate(names) if cy.flags >> b & 1)
            print(f"  {k}: pos {cy.pos} calls {len(cy.calls)} legal/stage {list(legal.values())} codes {codes} steps "
                  f"{int(cy.calls[:, 4].min())}-{int(cy.calls[:, 4].max())} winner #{cy.best_call} stage {st} v {cy.winner_vel} cost {cy.cost:.4f} "
                  f"pts {cy.n_points} flags {fl} within {len(cy.within)} pre {cy.pre} post {cy.post[:, 0]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--show", action="store_true")
    a = ap.parse_args()
    if not available():
        sys.exit("the reference base_local_planner / costmap_2d trees are not on this machine")
    with tempfile.TemporaryDirectory() as wd:
        d, cases = generate(wd)
    if a.show:
        show(d, cases)
    np.savez_compressed(a.out, **d)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, {len(d)} arrays, knife-edge minimum {json.loads(str(d['meta']))['knife_edge_min_cells']:.3e}")


if __name__ == "__main__":
    main()
