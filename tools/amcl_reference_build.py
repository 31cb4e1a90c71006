"""Compile the reference amcl core (amcl/src/amcl/{map,pf,sensors}) in place into a scratch directory, plus
tools/amcl_golden_harness.cpp, and run the harness.  Shared by tools/make_amcl_goldens.py and tests/test_amcl_reference.py.

amcl's core includes only the standard library.  One forced include is needed: modern libstdc++ rejects `abs(unsigned int)`
as ambiguous (map_cspace.cpp's enqueue); the shim restores what the old overload set resolved to.  The drawing helpers
(map_draw.c, pf_draw.c) need rtk and are left out.  The core is built as a release build (-DNDEBUG): the beam model asserts
pz <= 1.0, which amcl's own default mixture weights (laser_z_hit 0.95 + z_short + z_max + z_rand) can exceed.
"""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("NAVGPU_REFERENCE", "/root/reference")
AMCL = os.path.join(REFERENCE, "amcl")
SHIM = "#include <stdlib.h>\ninline int abs(unsigned int v) { return abs((int)v); }\n"
SOURCES = ["map/map.c", "map/map_range.c", "map/map_store.c", "map/map_cspace.cpp", "pf/pf.c", "pf/pf_kdtree.c", "pf/pf_pdf.c",
           "pf/pf_vector.c", "pf/eig3.c", "sensors/amcl_sensor.cpp", "sensors/amcl_laser.cpp", "sensors/amcl_odom.cpp"]


def available():
    return os.path.isdir(os.path.join(AMCL, "src", "amcl"))


def include_dirs():
    inc = os.path.join(AMCL, "include")
    return [inc] + [os.path.join(inc, "amcl", d) for d in ("map", "pf", "sensors")]


def build_core(workdir):
    """Objects of the reference core in workdir; returns their paths."""
    os.makedirs(workdir, exist_ok=True)
    shim = os.path.join(workdir, "abs_shim.h")
    with open(shim, "w") as f:
        f.write(SHIM)
    incs = sum((["-I", d] for d in include_dirs()), [])
    objs = []
    for rel in SOURCES:
        src = os.path.join(AMCL, "src", "amcl", rel)
        obj = os.path.join(workdir, rel.replace("/", "_") + ".o")
        if rel.endswith(".c"):
            cmd = ["gcc", "-O2", "-DNDEBUG", "-fPIC", "-w"] + incs + ["-c", src, "-o", obj]
        else:
            cmd = ["g++", "-O2", "-DNDEBUG", "-fPIC", "-w", "-include", shim] + incs + ["-c", src, "-o", obj]
        subprocess.run(cmd, check=True)
        objs.append(obj)
    return objs


def build_harness(workdir):
    objs = build_core(workdir)
    exe = os.path.join(workdir, "amcl_golden_harness")
    subprocess.run(["g++", "-O2", "-w"] + sum((["-I", d] for d in include_dirs()), []) +
                   [os.path.join(HERE, "amcl_golden_harness.cpp")] + objs + ["-o", exe, "-lm"], check=True)
    return exe


def build_adapter_harness(workdir, navgpu_root):
    """The same driver running navgpu::AMCLLaser (navigation_amd/amcl_adapter), linked with the reference core and libnavgpu.so."""
    objs = build_core(workdir)
    exe = os.path.join(workdir, "amcl_adapter_harness")
    adapter = os.path.join(navgpu_root, "navigation_amd", "amcl_adapter")
    libdir = os.path.join(navgpu_root, "navigation_amd")
    incs = sum((["-I", d] for d in include_dirs() + [adapter, os.path.join(navgpu_root, "include")]), [])
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unused-parameter", "-DNAVGPU_ADAPTER"] + incs +
                   [os.path.join(HERE, "amcl_golden_harness.cpp"), os.path.join(adapter, "navgpu_amcl_laser.cpp")] + objs +
                   ["-o", exe, "-L", libdir, "-l:libnavgpu.so", "-Wl,-rpath," + libdir, "-lm"], check=True)
    return exe


def run_cspace(exe, workdir, occ_state, scale, max_occ_dist):
    sy, sx = occ_state.shape
    p, o, out = (os.path.join(workdir, n) for n in ("cs_params.bin", "cs_occ.bin", "cs_out.bin"))
    np.array([sx, sy, scale, max_occ_dist], np.float64).tofile(p)
    np.ascontiguousarray(occ_state, np.int8).tofile(o)
    subprocess.run([exe, "cspace", p, o, out], check=True)
    return np.fromfile(out, np.float32).reshape(sy, sx)


PARAM_ORDER = ("model_type", "max_beams", "z_hit", "z_short", "z_max", "z_rand", "sigma_hit", "lambda_short", "chi_outlier", "do_beamskip",
               "beam_skip_distance", "beam_skip_threshold", "beam_skip_error_threshold", "gompertz_a", "gompertz_b", "gompertz_c",
               "input_shift", "input_scale", "output_shift", "off_map_factor", "non_free_space_factor", "non_free_space_radius",
               "alpha_slow", "alpha_fast")


def run_update(exe, workdir, occ_state, scale, origin, max_occ_dist, params, laser, w, converged, poses, weights, ranges, range_max):
    """One AMCLLaser::UpdateSensor.  origin: map_t origin_x / origin_y (centre); params: dict of PARAM_ORDER.
    -> (updated, w_slow, w_fast, weights, beam-skip error branch taken, ms spent in UpdateSensor, obs_count or None)
    (obs_count: the beam-skip counts of a converged likelihood-field-prob set with do_beamskip)"""
    sy, sx = occ_state.shape
    n, rc = len(poses), len(ranges)
    head = [sx, sy, scale, origin[0], origin[1], max_occ_dist] + [float(params[k]) for k in PARAM_ORDER] + list(laser) + \
        [w[0], w[1], converged, n, rc, range_max]
    p, o, out = (os.path.join(workdir, nm) for nm in ("up_params.bin", "up_occ.bin", "up_out.bin"))
    np.concatenate([np.array(head, np.float64), np.asarray(poses, np.float64).ravel(), np.asarray(weights, np.float64).ravel(),
                    np.asarray(ranges, np.float64).reshape(-1)]).tofile(p)
    np.ascontiguousarray(occ_state, np.int8).tofile(o)
    r = subprocess.run([exe, "update", p, o, out], check=True, capture_output=True, text=True)
    v = np.fromfile(out, np.float64)
    oc = v[4 + n:].astype(np.int32) if len(v) > 4 + n else None
    return int(v[0]), v[1], v[2], v[3:3 + n].copy(), "integrating all observations" in r.stderr, v[3 + n], oc
