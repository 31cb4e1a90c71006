#!/usr/bin/env python3
"""Write tests/golden/g17_costmap_reference.npz: costmap update cycles as the reference's own classes compute them.

tools/costmap_reference_harness.cpp compiles costmap_2d's LayeredCostmap, StaticLayer, ObstacleLayer, VoxelLayer, InflationLayer,
CostmapLayer, Layer, Costmap2D, ObservationBuffer, the footprint helpers and voxel_grid's VoxelGrid in place (NAVGPU_REFERENCE, against
tools/costmap_ref_stubs/, tools/dwa_ref_stubs/ and tests/ros_stubs/) and runs the cases of tests/costmap_reference_cases.py.  The file
holds inputs and reference outputs only: neither the CPU oracle nor the library is imported here.

Per case NAME (tests/costmap_reference_cases.py has the decoder), one entry per updateMap cycle in every array:
  NAME_in               the harness's input doubles: geometry, layers and their parameters, footprint, occupancy grid, per cycle the
                        pose, a footprint change and the observations (float32 points)
  NAME_origin           the master Costmap2D's origin after the cycle (float64)
  NAME_box              x0, xn, y0, yn: the box updateMap handed to the layers' updateCosts (LayeredCostmap::getBounds)
  NAME_layer            the obstacle / voxel layer's own grid
  NAME_voxels           the voxel grid's uint32 words, for the cycles meta["voxel_cycles"][NAME] lists
  NAME_master_static, NAME_master_obstacle   the master grid behind that layer's updateCosts, where another layer follows
  NAME_master           the master grid after the cycle
  NAME_inscribed        LayeredCostmap::getInscribedRadius() (float64), with an inflation layer
  NAME_cost_table       InflationLayer::computeCost(hypot(i, j)), i, j <= R + 1: what cached_costs_ holds
  NAME_master_exact     NOT a reference output: the order-independent exact-distance specification, built here in numpy
                        (costmap_reference_cases.exact_masters / inflate_exact) from NAME_cost_table and the master grid in front of the
                        inflation layer; outside a cycle's box it carries its own earlier cycles, as a costmap inflated this way would
meta (JSON): compile flags, the sources compiled in place, the case names, voxel_cycles, and per inflation case whether the reference's
priority-queue walk and the specification give the same grid in every cycle (walk_equals_exact).
Usage: python tools/make_costmap_goldens.py [--out PATH]
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
import costmap_reference_cases as K  # noqa: E402

REFERENCE = os.environ.get("NAVGPU_REFERENCE", "/root/reference")
OUT = K.GOLDEN
FLAGS = ["-std=c++14", "-O2", "-w", "-ffp-contract=off"]
PLUGINS = ["static_layer", "obstacle_layer", "voxel_layer", "inflation_layer"]
COSTMAP = ["layered_costmap", "layer", "costmap_layer", "costmap_2d", "footprint", "costmap_math", "observation_buffer", "array_parser"]


def sources():
    return ([os.path.join(REFERENCE, "costmap_2d", "plugins", s + ".cpp") for s in PLUGINS] +
            [os.path.join(REFERENCE, "costmap_2d", "src", s + ".cpp") for s in COSTMAP] +
            [os.path.join(REFERENCE, "voxel_grid", "src", "voxel_grid.cpp")])


def available():
    return all(os.path.isfile(s) for s in sources())


def build_harness(workdir):
    exe = os.path.join(workdir, "costmap_reference_harness")
    inc = [os.path.join(HERE, "costmap_ref_stubs"), os.path.join(HERE, "dwa_ref_stubs"), os.path.join(ROOT, "tests", "ros_stubs")] + [
        os.path.join(REFERENCE, p, "include") for p in ("costmap_2d", "voxel_grid", "nav_core")]
    cmd = ["g++"] + FLAGS + [a for i in inc for a in ("-I", i)] + [os.path.join(HERE, "costmap_reference_harness.cpp")] + sources() + [
        "-o", exe, "-lpthread", "-lm"]
    subprocess.run(cmd, check=True)
    return exe


def run_harness(exe, workdir, cases):
    fin, fout = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(fin, "wb") as f:
        np.array([len(cases)], np.int64).tofile(f)
        for c in cases:
            d = K.encode_input(c)
            np.array([len(d)], np.int64).tofile(f)
            d.tofile(f)
    subprocess.run([exe, fin, fout], check=True)
    raw = np.fromfile(fout, np.uint8)
    out, at = [], 0
    for c in cases:
        n = int(raw[at:at + 8].view(np.int64)[0])
        out.append(K.decode_output(raw[at + 8:at + 8 + n], c))
        at += 8 + n
    assert at == len(raw)
    return out


def generate(workdir):
    cases = K.build_cases()
    exe = build_harness(workdir)
    outs = run_harness(exe, workdir, cases)
    d, voxel_cycles, walk_equals_exact = {}, {}, {}
    for c, recs in zip(cases, outs):
        name = c["name"]
        st = K.stages(c)
        d[name + "_in"] = K.encode_input(c)
        d[name + "_origin"] = np.stack([r["origin"] for r in recs])
        d[name + "_box"] = np.stack([r["box"] for r in recs])
        d[name + "_master"] = np.stack([r["master_" + st[-1]] for r in recs])
        for s in st[:-1]:
            d[f"{name}_master_{s}"] = np.stack([r["master_" + s] for r in recs])
        if c["obstacle"] is not None:
            d[name + "_layer"] = np.stack([r["layer"] for r in recs])
            if c["obstacle"]["voxel"]:
                cycles = list(range(len(recs)))  # (a case may list its last cycle only, should the file outgrow its bound)
                voxel_cycles[name] = cycles
                d[name + "_voxels"] = np.stack([recs[k]["voxels"] for k in cycles])
        if c["inflation"] is not None:
            d[name + "_cost_table"] = np.stack([r["cost_table"] for r in recs])
            d[name + "_inscribed"] = np.array([r["inscribed"] for r in recs], np.float64)
            exact = np.stack(K.exact_masters(c, recs))
            d[name + "_master_exact"] = exact
            walk_equals_exact[name] = bool(np.array_equal(exact, d[name + "_master"]))
    meta = dict(
        flags=" ".join(FLAGS),
        compiled_in_place=[os.path.relpath(s, REFERENCE) for s in sources()],
        cases=[c["name"] for c in cases],
        voxel_cycles=voxel_cycles,
        walk_equals_exact=walk_equals_exact,
        master_exact="a specification built from the reference's cost table (NAME_cost_table) by costmap_reference_cases.exact_masters: every cell "
                     "takes the cost of its nearest lethal cell; it is not a reference output.  NAME_master is the reference's priority-queue walk.")
    d["meta"] = np.array(json.dumps(meta, sort_keys=True))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference costmap_2d / voxel_grid trees are not on this machine")
    with tempfile.TemporaryDirectory() as wd:
        d = generate(wd)
    np.savez_compressed(a.out, **d)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, {len(d)} arrays")


if __name__ == "__main__":
    main()
