#!/usr/bin/env python3
"""Write tests/golden/g13_global_plan.npz: the global-plan tests' inputs (tests/global_plan_ref.py: batch_cases, serpentine_cases,
short_cases), what the CPU oracle's global_planner core makes of them, and what the reference's own
OrientationFilter::processPath (global_planner/src/orientation_filter.cpp compiled in place, driven by
tools/global_plan_harness.cpp) leaves as orientations in its four modes.

Per case set S (batch, serpentine, short) and parameter variant V:
  S_frames, S_starts, S_goals, S_maps (+ S_map_index)     the inputs
  S_V_status, S_V_counts                                  status and n_poses per plan
  S_V_path                                                the oracle's traceback points (float32, goal first), concatenated; for `batch`
                                                          tests/test_global_planner_reference.py gets the same bits from the reference's classes
  S_V_plan                                                the assembled world plan before the filter: {x, y, yaw}, concatenated
  S_V_quat                                                4 x total x {z, w}: the reference's quaternions per orientation mode
  S_V_grid, S_V_max                                       publishPotential's bytes and maximum (scale 100) of the plans attempted
tf and angles are not in the reference tree: their formulas are in tools/global_plan_stubs/.
Usage: python tools/make_global_plan_goldens.py [--out PATH]
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
import global_plan_ref as R  # noqa: E402

REFERENCE = os.environ.get("NAVGPU_REFERENCE", "/root/reference")
GP = os.path.join(REFERENCE, "global_planner")
OUT = os.path.join(ROOT, "tests", "golden", "g13_global_plan.npz")
VARIANTS = {"default": dict(), "grid": dict(use_grid_path=1), "old": dict(old_navfn_behavior=1), "linear": dict(use_quadratic=0)}
SETS = {"batch": ("default", "grid", "old", "linear"), "serpentine": ("default",), "short": ("default", "grid", "old")}


def available():
    return os.path.isfile(os.path.join(GP, "src", "orientation_filter.cpp"))


def case_set(name):
    if name == "batch":
        return R.batch_cases()[0]
    return R.serpentine_cases()[:1] if name == "serpentine" else R.short_cases()


def build_harness(workdir):
    exe = os.path.join(workdir, "global_plan_harness")
    subprocess.run(["g++", "-O2", "-w", "-ffp-contract=off", "-I", os.path.join(HERE, "global_plan_stubs"), "-I", os.path.join(ROOT, "tests", "ros_stubs"),
                    "-I", os.path.join(GP, "include"), os.path.join(HERE, "global_plan_harness.cpp"),
                    os.path.join(GP, "src", "orientation_filter.cpp"), "-o", exe, "-lm"], check=True)
    return exe


def run_harness(exe, workdir, plans):
    """plans: list of (start_yaw, (n, 3) poses) -> list of (4, n, 2) quaternion {z, w} arrays"""
    fin, fout = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(fin, "wb") as f:
        np.array([len(plans)], np.int64).tofile(f)
        for start_yaw, poses in plans:
            np.array([len(poses)], np.int64).tofile(f)
            np.array([start_yaw], np.float64).tofile(f)
            np.ascontiguousarray(poses, np.float64).tofile(f)
    subprocess.run([exe, fin, fout], check=True)
    v = np.fromfile(fout, np.float64)
    out, at = [], 0
    for _, poses in plans:
        n = len(poses)
        out.append(v[at:at + 8 * n].reshape(4, n, 2).copy())
        at += 8 * n
    assert at == len(v)
    return out


def generate(workdir):
    from oracle import pyoracle as orc
    core = R.oracle_core(orc)
    exe = build_harness(workdir)
    d = {}
    for name, variants in SETS.items():
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
        for v in variants:
            kw = VARIANTS[v]
            refs = [R.make_plan(core, *c, R.NONE, **kw) for c in cases]
            key = f"{name}_{v}_"
            d[key + "status"] = np.array([r["status"] for r in refs], np.int32)
            d[key + "counts"] = np.array([r["n_poses"] for r in refs], np.int32)
            made = [(c[2][2], r["poses"]) for c, r in zip(cases, refs) if r["n_poses"]]
            d[key + "path"] = np.concatenate([r["path"] for r in refs if r["n_poses"]]).astype(np.float32)
            d[key + "plan"] = np.concatenate([p for _, p in made])
            d[key + "quat"] = np.concatenate(run_harness(exe, workdir, made), axis=1)
            grids = [R.potential_grid(r["potential"], 100) for r in refs if r["potential"] is not None]
            d[key + "grid"] = np.stack([g for g, _ in grids])
            d[key + "max"] = np.array([m for _, m in grids], np.float32)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if not available():
        sys.exit("the reference global_planner tree is not on this machine")
    with tempfile.TemporaryDirectory() as wd:
        d = generate(wd)
    np.savez_compressed(a.out, **d)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, {len(d)} arrays")


if __name__ == "__main__":
    main()
