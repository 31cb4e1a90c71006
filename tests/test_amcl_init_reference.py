"""CPU checks of the init yardstick: tests/golden/g12_amcl_init.npz is what the reference amcl core (compiled in place) computes
for pf_init and for pf_init_model with the node's uniformPoseGenerator; a Python restatement of the drand48 candidate stream and
of the acceptance chain reproduces every case's chosen candidates and final state; the near-tie margin holds; the file is small
and covers the cases the device is checked on."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import amcl_reference_build as B  # noqa: E402
import make_amcl_init_goldens as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g12_amcl_init.npz")
needs_reference = pytest.mark.skipif(not B.available(), reason="the reference amcl tree is not on this machine")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@needs_reference
def test_init_goldens_reproduce_from_the_reference(tmp_path, golden):
    out = tmp_path / "g12.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_amcl_init_goldens.py"), "--out", str(out)], check=True,
                   capture_output=True)
    new = np.load(out)
    assert sorted(new.files) == sorted(golden.files)
    for k in golden.files:
        assert np.array_equal(golden[k], new[k], equal_nan=golden[k].dtype.kind == "f"), k


def test_python_streams_reproduce_every_case(golden):
    for n in golden["gauss_cases"]:
        n = str(n)
        ms, seed = int(golden[n + "_in"][0]), int(golden[n + "_in"][1])
        st = golden[n + "_state"]
        assert int(st[0]) == G.drand48_state(seed)
        assert int(st[1]) == G.gauss_consumed(int(st[0]), 3 * ms), n
    for n in golden["uniform_cases"]:
        n = str(n)
        i = golden[n + "_in"]
        ms, thr, mult, has_scan = int(i[1]), i[2], i[3], int(i[4])
        st, used = golden[n + "_state"], int(golden[n + "_used"][0])
        chosen = golden[n + "_chosen"]
        if G.scored(dict(has_scan=has_scan, threshold=thr, multiplier=mult)):
            ref, _ = G.chain(golden[n + "_scores"], ms, thr, mult)
            assert list(ref) == list(chosen) and ref[-1] == used - 1, n
        else:
            assert used == ms and list(chosen) == list(range(ms)), n
        assert int(st[1]) == G.advance(int(st[0]), 2 * used), n
        # the chosen poses are the stream's candidates: cell from value 2j, theta from value 2j + 1
        geo = golden[f"map{int(i[0])}_geom"]
        occ = golden[f"map{int(i[0])}_occ"]
        P = golden[n + "_poses"]
        x = int(st[0])
        vals = []
        for _ in range(2 * used):
            x = (G.A * x + G.C) % G.M
            vals.append(x / float(G.M))
        th = np.array(vals[1::2])[chosen] * 2 * math.pi - math.pi
        assert np.array_equal(P[:, 2], th), n
        sy, sx = occ.shape
        ci = np.rint((P[:, 0] - geo[1]) / geo[0]).astype(int) + sx // 2
        cj = np.rint((P[:, 1] - geo[2]) / geo[0]).astype(int) + sy // 2
        assert np.all(occ[cj, ci] == -1), n


def test_near_tie_margin_holds(golden):
    for n in golden["uniform_cases"]:
        n = str(n)
        i = golden[n + "_in"]
        if not G.scored(dict(has_scan=int(i[4]), threshold=i[2], multiplier=i[3])):
            continue
        _, margin = G.chain(golden[n + "_scores"], int(i[1]), i[2], i[3])
        assert margin > G.MARGIN and margin == golden[n + "_margin"][0], n


def test_file_is_small_and_covers_the_cases(golden):
    assert os.path.getsize(GOLDEN) < 600 * 1024
    g = set(map(str, golden["gauss_cases"]))
    u = set(map(str, golden["uniform_cases"]))
    assert any(n.startswith("gauss_diag") for n in g) and any(n.startswith("gauss_full") for n in g)
    assert any(np.any(np.diag(golden[n + "_in"][5:].reshape(3, 3)) == 0) for n in g)
    assert len({int(golden[n + "_in"][0]) for n in g}) >= 3
    for m in ("beam", "lf", "prob", "gompertz"):
        for mult in ("0.0", "0.5", "0.9"):
            assert f"scored_{m}_{mult}" in u
    for n in ("unscored", "disabled_threshold0", "disabled_multiplier1", "disabled_multiplier_neg", "disabled_no_scan", "radius",
              "golden_map0", "golden_map1", "golden_map2"):
        assert n in u
