"""CPU checks of the motion-model yardstick: tests/golden/g11_amcl_motion.npz is what the reference amcl core (compiled in place)
computes, a pure-Python restatement of pf_ran_gaussian's drand48 consumption reproduces every case's final state, and the
drop-in adapter (navgpu::AMCLOdom) builds against the reference's headers and core, bridges the drand48 state without
disturbing it, and has no CPU fallback."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import amcl_reference_build as B  # noqa: E402
import make_amcl_motion_goldens as G  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g11_amcl_motion.npz")
needs_reference = pytest.mark.skipif(not B.available(), reason="the reference amcl tree is not on this machine")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@needs_reference
def test_motion_goldens_reproduce_from_the_reference(tmp_path, golden):
    out = tmp_path / "g11.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_amcl_motion_goldens.py"), "--out", str(out)], check=True,
                   capture_output=True)
    new = np.load(out)
    assert sorted(new.files) == sorted(golden.files)
    for k in golden.files:
        eq_nan = golden[k].dtype.kind == "f"
        assert np.array_equal(golden[k], new[k], equal_nan=eq_nan), k


def test_python_gaussian_stream_matches_the_reference_consumption(golden):
    for name in golden["cases"]:
        name = str(name)
        s_in, s_out = (int(v) for v in golden[name + "_state"])
        n = int(golden[name + "_count"][0])
        got, recs = G.gauss_stream(s_in, 3 * n)
        assert got == s_out, name
        assert len(recs) == 3 * n


def test_zero_draw_states_draw_an_exact_zero():
    for j in (1, 7, 2048, 2049):
        x = G.state_drawing_zero_at(j)
        for _ in range(j):
            x = (G.A * x + G.C) % G.M
        assert x == 0
    # the zero is skipped: the stream after it pairs the next nonzero value
    s = G.state_drawing_zero_at(1)
    x1 = (G.A * ((G.A * s + G.C) % G.M) + G.C) % G.M
    _, recs = G.gauss_stream(s, 1)
    assert recs and x1 != 0


def test_drand48_replay_is_the_documented_generator():
    from navigation_amd.localization import drand48_state
    assert drand48_state(0) == G.drand48_state(0) == 0x330E
    x1 = (0x5DEECE66D * 0x330E + 0xB) % (1 << 48)
    assert G.gauss_stream(0x330E, 0)[0] == 0x330E
    assert (G.A * 0x330E + G.C) % G.M == x1


def test_golden_file_stays_small():
    assert os.path.getsize(GOLDEN) < 600 * 1024


def test_golden_cases_cover_the_issue_list(golden):
    names = {str(n) for n in golden["cases"]}
    for m in ("diff", "omni", "diff_corr", "omni_corr", "gauss"):
        for c in ("forward", "inplace", "backward", "across_pi", "zero_motion"):
            assert f"{m}_{c}" in names
    for c in ("gauss_no_abs", "diff_corr_negative_alpha", "zero_draw_at_7", "zero_draw_at_2048", "zero_draw_at_2049", "empty", "partial",
              "large_diff"):
        assert c in names
    assert golden["large_diff_count"][0] == 5000
    assert golden["partial_count"][0] < len(golden["partial_poses_in"])
    assert golden["empty_count"][0] == 0 and golden["empty_state"][0] == golden["empty_state"][1]
    assert np.isnan(golden["diff_corr_negative_alpha_poses_out"]).any()
    for m in ("diff", "omni", "gauss"):   # zero motion: every sigma 0, the poses do not move, the draws are still consumed
        n = f"{m}_zero_motion"
        assert np.array_equal(golden[n + "_poses_out"], golden[n + "_poses_in"])
        assert golden[n + "_state"][0] != golden[n + "_state"][1]
    assert np.any(golden["gauss_forward_odom"][6:] != 0)


@needs_reference
def test_adapter_builds_against_the_reference_bridges_the_state_and_has_no_cpu_fallback(tmp_path, golden):
    """navigation_amd/amcl_adapter/navgpu_amcl_odom.cpp compiled against the reference's amcl headers and include/navgpu.h, linked
    with the reference core and libnavgpu.so.  The seed48 bridge reads the state and puts it back without changing the next
    drand48().  Without a GPU construction reports NAVGPU_ERR_NO_DEVICE; with one, the update equals the reference's golden."""
    import navigation_amd as nav
    if not os.path.exists(nav.lib_path()):
        nav.build()
    exe = G.build_adapter_harness(str(tmp_path), ROOT)
    for x in (0x330E, 0x123456789ABC, (1 << 48) - 1):
        r = subprocess.run([exe, "bridge", str(x)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.split() == ["bridge", "ok", str(x)], r.stderr
    name = "diff_forward"
    args = (exe, str(tmp_path), golden[name + "_params"], golden[name + "_odom"], int(golden[name + "_state"][0]),
            int(golden[name + "_count"][0]), golden[name + "_poses_in"])
    if nav.lib().navgpu_device_count() <= 0:
        with pytest.raises(subprocess.CalledProcessError) as e:
            G.run_update(*args)
        assert e.value.returncode == 3
        assert "navgpu status -2" in e.value.stderr and "no usable HIP device" in e.value.stderr
    else:
        st, _, P = G.run_update(*args)
        assert st == int(golden[name + "_state"][1])
        assert np.allclose(P, golden[name + "_poses_out"], rtol=1e-12, atol=1e-12)
