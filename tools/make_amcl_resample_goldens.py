#!/usr/bin/env python3
"""Write tests/golden/g10_amcl_resample.npz from the reference amcl core itself (pf/ compiled in place, see
tools/amcl_reference_build.py, driven by tools/amcl_resample_harness.cpp).

Each case creates its set with pf_init_model from a pose list (max_samples poses), overwrites the weights and w_slow / w_fast,
calls srand48(seed) and runs pf_update_resample once; random_pose_fn pops a recorded pool, so the only drand48() draws are the
resampler's.  drand48 is the documented 48-bit LCG (a = 0x5DEECE66D, c = 0xB, state seed << 16 | 0x330E): this tool replays it
into the per-candidate {u_flag, u_pick} stream (multinomial: u_flag, then u_pick unless the candidate is random) or the one
systematic_sample_start, and checks the replay against the next drand48() value the driver reports after the call.

The file holds what each call reads and what it produces: the pool poses it popped, the {u_flag, u_pick} pairs of the candidates
it drew, and the new set as row indices into [poses_in; pool] (its poses are copies; its weights, all 1 / n, are checked here and
not stored).  Poses whose bin coordinate pose / {0.5, 0.5, 10 deg} lies within 1e-9 of an integer are redrawn (both sides divide in IEEE fp64,
so this only guards the histogram key against any future change of that expression).  Reference clusters are stored in the
device's documented order: by the lowest sample index they hold.  The reference's single-thread time per call is printed.
Usage: python tools/make_amcl_resample_goldens.py [--out PATH]
"""
import argparse
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import amcl_reference_build as B  # noqa: E402

ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden", "g10_amcl_resample.npz")
SIZE = np.array([0.5, 0.5, 10 * math.pi / 180])
MARGIN = 1e-9


def build_harness(workdir):
    objs = B.build_core(workdir)
    exe = os.path.join(workdir, "amcl_resample_harness")
    subprocess.run(["g++", "-O2", "-w"] + sum((["-I", d] for d in B.include_dirs()), []) +
                   [os.path.join(HERE, "amcl_resample_harness.cpp")] + objs + ["-o", exe, "-lm"], check=True)
    return exe


class Drand48:
    A, C, M = 0x5DEECE66D, 0xB, 1 << 48

    def __init__(self, seed):
        self.x = ((seed & 0xFFFFFFFF) << 16) | 0x330E

    def __call__(self):
        self.x = (self.A * self.x + self.C) % self.M
        return self.x / float(self.M)


def replay(model, seed, w_diff, max_samples):
    """-> (u (max_samples, 2), systematic_start, generator positioned after what the reference consumed is decided later)"""
    g = Drand48(seed)
    u = np.ones((max_samples, 2))
    if model == 1:
        return u, g(), [g()]
    seq = []
    for k in range(max_samples):
        u[k, 0] = g()
        seq.append(("f", k))
        if not u[k, 0] < w_diff:
            u[k, 1] = g()
            seq.append(("p", k))
    seq_vals = [u[k, 0] if t == "f" else u[k, 1] for t, k in seq] + [g()]
    return u, None, seq_vals


def near_boundary(p):
    f = p / SIZE
    return (np.abs(f - np.round(f)) < MARGIN).any(1)


def fix(rng, p):
    while True:
        bad = near_boundary(p)
        if not bad.any():
            return p
        p[bad] += rng.normal(0, 1e-4, size=(bad.sum(), 3))


def blob(rng, n, centre, sd):
    return np.asarray(centre, float) + rng.normal(0, 1, size=(n, 3)) * np.asarray(sd, float)



def make_cases(rng):
    """name -> dict(model, min, max, ws, wf, poses, weights, pool, seed)"""
    C = {}

    def add(name, model, poses, weights=None, ws=0.001, wf=0.001, mn=50, pool=None, pop_err=0.01, pop_z=3.0, dist=0.5):
        n = len(poses)
        poses = fix(rng, np.asarray(poses, float))
        if weights is None:
            weights = rng.uniform(0.5, 1.5, n)
            weights /= weights.sum()
        if pool is None:
            pool = np.stack([rng.uniform(-6, 6, n), rng.uniform(-6, 6, n), rng.uniform(-math.pi, math.pi, n)], 1)
        C[name] = dict(model=model, min=mn, max=n, ws=ws, wf=wf, poses=poses, weights=np.asarray(weights, float), pool=fix(rng, pool),
                       seed=int(rng.integers(1, 2 ** 31 - 1)), pop_err=pop_err, pop_z=pop_z, dist=dist)

    spread = lambda n: np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(-math.pi, math.pi, n)], 1)  # noqa: E731
    for model, tag in ((0, "multi"), (1, "sys")):
        add(f"{tag}_wdiff0_manybins", model, spread(300))                                     # hundreds of bins: the limit is max
        # a dozen bins and pop_err 0.05: the KLD limit binds far below max_samples
        add(f"{tag}_kld_binds", model, blob(rng, 600, (1.1, 1.1, 0.2), (0.15, 0.15, 0.03)), pop_err=0.05)
        add(f"{tag}_wdiff_pos", model, blob(rng, 500, (1.0, 2.0, 0.3), (0.3, 0.3, 0.2)), ws=0.002, wf=0.0013)
        one = np.array([0.05, 0.05, 0.01]) + rng.uniform(0, 1, size=(300, 3)) * [0.4, 0.4, 0.15]  # one bin: the limit is max_samples
        add(f"{tag}_one_bin", model, one)
        few = np.array([0.05, 0.05, 0.01]) + rng.uniform(0, 1, size=(400, 3)) * [0.4, 0.4, 0.3]  # two bins: limit 106 -> min 200
        add(f"{tag}_min_clamp", model, few, mn=200, pop_err=0.05)
        sep = np.concatenate([blob(rng, 150, (-4, -3, 1.0), (0.1, 0.1, 0.05)), blob(rng, 150, (3, 2, -2.0), (0.1, 0.1, 0.05)),
                              blob(rng, 150, (0.5, 4, 0.0), (0.1, 0.1, 0.05))])
        add(f"{tag}_separated", model, sep[rng.permutation(len(sep))])
        # bins touching only diagonally (x, y) and the theta bins either side of +-pi (no wrap: two clusters)
        diag = []
        for i, (bx, by, th) in enumerate([(0, 0, 0.3), (1, 1, 0.3), (2, 2, 0.3), (5, 0, 0.3), (6, -1, 0.3), (-3, 3, math.pi - 0.02),
                                          (-3, 3, -math.pi + 0.02)]):
            q = np.zeros((50, 3))
            q[:, 0] = bx * 0.5 + rng.uniform(0.05, 0.45, 50)
            q[:, 1] = by * 0.5 + rng.uniform(0.05, 0.45, 50)
            q[:, 2] = th + rng.uniform(-0.01, 0.01, 50)
            diag.append(q)
        diag = np.concatenate(diag)
        add(f"{tag}_diagonal_pi", model, diag[rng.permutation(len(diag))])
        add(f"{tag}_converged", model, blob(rng, 300, (2.0, -1.0, 0.5), (0.05, 0.05, 0.1)), dist=0.5)
        add(f"{tag}_unconverged", model, blob(rng, 300, (2.0, -1.0, 0.5), (0.6, 0.6, 0.1)), dist=0.5)
    # a set larger than w_diff leaves room for: new_count * (1 + w_diff) is capped at max_samples
    add("sys_capped", 1, blob(rng, 450, (0.0, 0.0, 0.0), (1.0, 1.0, 0.5)), ws=0.002, wf=0.0006)
    add("multi_capped", 0, blob(rng, 450, (0.0, 0.0, 0.0), (1.0, 1.0, 0.5)), ws=0.002, wf=0.0006)
    return C


def run(exe, td, c):
    inp, out = os.path.join(td, "rs_in.bin"), os.path.join(td, "rs_out.bin")
    head = [c["model"], c["min"], c["max"], c["pop_err"], c["pop_z"], c["dist"], c["ws"], c["wf"], c["seed"], len(c["pool"])]
    np.concatenate([np.array(head, np.float64), c["poses"].ravel(), c["weights"], c["pool"].ravel()]).tofile(inp)
    subprocess.run([exe, inp, out], check=True)
    v = np.fromfile(out, np.float64)
    leaf_in, n, ws, wf, leaf, ncl, conv, used, nxt, ms = v[:10]
    n, ncl = int(n), int(ncl)
    q = 10
    poses = v[q:q + 3 * n].reshape(n, 3)
    q += 3 * n
    weights = v[q:q + n]
    q += n
    cl_of = v[q:q + n].astype(np.int64)
    q += n
    cl = v[q:q + 14 * ncl].reshape(ncl, 14)
    q += 14 * ncl
    st = v[q:q + 12]
    return dict(leaf_in=int(leaf_in), n=n, ws=ws, wf=wf, leaf=int(leaf), ncl=ncl, conv=int(conv), used=int(used), next=nxt, ms=ms,
                poses=poses, weights=weights, cl_of=cl_of, cl=cl, st=st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if not B.available():
        sys.exit(f"the reference amcl tree is not at {B.AMCL}")
    rng = np.random.default_rng(10)
    cases = make_cases(rng)
    G = {"cases": np.array(sorted(cases))}
    with tempfile.TemporaryDirectory() as td:
        exe = build_harness(td)
        for name in sorted(cases):
            c = cases[name]
            R = run(exe, td, c)
            w_diff = max(1.0 - c["wf"] / c["ws"], 0.0)  # w_slow > 0 in every case: 0 / 0 is undefined for the systematic model
            u, start, stream = replay(c["model"], c["seed"], w_diff, c["max"])
            # the replay must put the reference's next draw right after what it consumed
            if c["model"] == 1:
                assert stream[0] == R["next"], name
                consumed = 1
            else:
                k = R["n"]
                rnd = int((u[:k, 0] < w_diff).sum())
                consumed = 2 * k - rnd
                assert stream[consumed] == R["next"], name
            # reference clusters in the documented order: by the lowest sample index they hold
            first = {}
            for i, cid in enumerate(R["cl_of"]):
                first.setdefault(int(cid), i)
            order = sorted(first, key=first.get)
            assert len(order) == R["ncl"], name
            key = name + "_"
            G[key + "params"] = np.array([c["model"], c["min"], c["max"], c["pop_err"], c["pop_z"], c["dist"], c["ws"], c["wf"], c["seed"]])
            # only what the call reads: the pool poses it popped, the draws of the candidates it drew
            pool = c["pool"][:R["used"]]
            G[key + "poses_in"], G[key + "weights_in"], G[key + "pool"] = c["poses"], c["weights"], pool
            G[key + "u"] = u[:R["n"]] if c["model"] == 0 else np.zeros((0, 2))
            G[key + "systematic_start"] = np.array([start if start is not None else 0.0])
            G[key + "out"] = np.array([R["leaf_in"], R["n"], R["ws"], R["wf"], R["leaf"], R["ncl"], R["conv"], R["used"]], np.float64)
            # the new set's poses are copies: stored as rows of [poses_in; pool]; its weights are all 1 / n (checked here)
            rows = {tuple(r): i for i, r in enumerate(np.concatenate([c["poses"], pool]))}
            src = np.array([rows[tuple(r)] for r in R["poses"]], np.int32)
            assert np.array_equal(np.concatenate([c["poses"], pool])[src], R["poses"]), name
            assert np.all(R["weights"] == 1.0 / R["n"]), name
            G[key + "src"] = src
            G[key + "clusters"] = R["cl"][order]
            G[key + "set_stats"] = R["st"]
            print(f"{name}: n={R['n']} leaf_in={R['leaf_in']} leaf={R['leaf']} clusters={R['ncl']} converged={R['conv']} "
                  f"random={R['used']} draws={consumed} ({R['ms']:.3f} ms)")
        # the reference's single-thread time per call at amcl_node's default size (5 000 particles)
        for model in (0, 1):
            c = dict(cases["multi_wdiff0_manybins"])
            n = 5000
            c.update(model=model, max=n, min=100, poses=np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n),
                                                                   rng.uniform(-math.pi, math.pi, n)], 1),
                     weights=np.full(n, 1.0 / n), pool=np.zeros((n, 3)))
            c["poses"][: n // 2] = blob(rng, n // 2, (1, 1, 0), (0.2, 0.2, 0.1))
            ts = [run(exe, td, c)["ms"] for _ in range(5)]
            print(f"reference {'systematic' if model else 'multinomial'}: {np.median(ts):.3f} ms per pf_update_resample "
                  f"(5000 particles, one thread)")
    np.savez_compressed(args.out, **G)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
