"""CPU checks of the amcl laser update's yardsticks: tests/golden/g9_amcl.npz is what the reference amcl core (compiled in place)
computes, the exact distance-transform specification against the reference's brushfire, the ctypes mirror of
navgpu_amcl_laser_params, the drop-in adapter (navgpu::AMCLLaser) built against the reference's headers and core, and the
no-CPU-fallback rule for the new handle and the adapter."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import amcl_reference_build as B  # noqa: E402
import amcl_spec as S  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g9_amcl.npz")
# measured on the golden maps (DESIGN "amcl"): 0.7 %, 1.7 %, 2.2 % of cells differ; the bound leaves room for nothing else
CSPACE_DIFF_BOUND = 0.03

needs_reference = pytest.mark.skipif(not B.available(), reason="the reference amcl tree is not on this machine")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@needs_reference
def test_goldens_reproduce_from_the_reference(tmp_path):
    out = tmp_path / "g9.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_amcl_goldens.py"), "--out", str(out)], check=True,
                   capture_output=True)
    new, old = np.load(out), np.load(GOLDEN)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        a, b = old[k], new[k]
        if a.dtype.kind == "f":
            assert np.array_equal(a, b, equal_nan=True), k
        else:
            assert np.array_equal(a, b), k


@needs_reference
def test_reference_cspace_of_a_random_map_is_above_the_exact_transform(tmp_path):
    exe = B.build_harness(str(tmp_path))
    rng = np.random.default_rng(7)
    occ = np.where(rng.random((160, 230)) < 0.01, 1, -1).astype(np.int8)
    occ[rng.random(occ.shape) < 0.02] = 0
    ref = B.run_cspace(exe, str(tmp_path), occ, 0.05, 1.0)
    ex = S.exact_cspace(occ, 0.05, 1.0)
    assert (ref >= ex).all()
    assert (ref != ex).mean() <= CSPACE_DIFF_BOUND


def test_exact_spec_against_golden_reference_maps(golden):
    for m in range(3):
        g = golden[f"map{m}_geom"]
        occ = S.convert_map(golden[f"map{m}_data"], int(g[3]))
        ref = golden[f"map{m}_dist"]
        ex = S.exact_cspace(occ, g[9], g[6])
        assert np.array_equal(ex, S.brute_cspace(occ, g[9], g[6]))
        assert (ref >= ex).all(), m
        frac = (ref != ex).mean()
        print(f"map{m}: {100 * frac:.2f} % of cells differ from the exact transform, max {np.abs(ref - ex).max():.4f} m")
        assert frac <= CSPACE_DIFF_BOUND


def test_golden_cases_cover_the_branches(golden):
    cfgs = list(golden["configs"])
    assert {"beam", "field", "prob", "prob_skip", "prob_skip_error", "gompertz"} <= set(cfgs)
    for m in range(3):
        assert golden[f"prob_skip_error_m{m}_out"][3] == 1.0
        assert golden[f"prob_skip_m{m}_out"][3] == 0.0
        scan = golden[f"field_m{m}_scan"]
        assert np.isnan(scan[:, 0]).any() and (scan[:, 0] >= 4.0).any()
    data = golden["map0_data"]
    assert {0, 100, -1, 50} <= set(np.unique(data).tolist())
    assert golden["map1_geom"][3] == 2 and golden["map0_data"].shape[0] != golden["map0_data"].shape[1]


def test_laser_params_mirror_matches_header(tmp_path):
    from navigation_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "navgpu.h"\nint main(){printf("%zu %zu %zu %zu\\n",'
                   'sizeof(navgpu_amcl_laser_params),offsetof(navgpu_amcl_laser_params,do_beamskip),'
                   'offsetof(navgpu_amcl_laser_params,beam_skip_distance),offsetof(navgpu_amcl_laser_params,alpha_fast));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = _lib.AmclLaserParams
    assert got == [C.sizeof(P), P.do_beamskip.offset, P.beam_skip_distance.offset, P.alpha_fast.offset]
    assert set(B.PARAM_ORDER) == {f[0] for f in P._fields_} - {"reserved"}


def test_amcl_handle_has_no_cpu_fallback():
    import navigation_amd as nav
    if not os.path.exists(nav.lib_path()):
        nav.build()
    L = nav.lib()
    if L.navgpu_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(nav.NavgpuError) as e:
        nav.AmclLaser(2, 100, 30)
    assert "no usable HIP device" in str(e.value)


@needs_reference
def test_adapter_builds_against_the_reference_and_has_no_cpu_fallback(tmp_path, golden):
    """navigation_amd/amcl_adapter compiled against the reference's amcl headers and include/navgpu.h, linked with the reference
    core and libnavgpu.so, driven like amcl_node drives amcl::AMCLLaser.  Without a GPU its construction reports
    NAVGPU_ERR_NO_DEVICE; with one, the update equals the reference's golden."""
    import navigation_amd as nav
    if not os.path.exists(nav.lib_path()):
        nav.build()
    exe = B.build_adapter_harness(str(tmp_path), ROOT)
    name, m = "field_factors", 2
    g = golden[f"map{m}_geom"]
    occ = S.convert_map(golden[f"map{m}_data"], int(g[3]))
    params = {str(k): v for k, v in zip(golden["param_order"], golden[f"{name}_params"])}
    st = golden[f"{name}_m{m}_state_in"]
    args = (exe, str(tmp_path), occ, g[9], (g[7], g[8]), g[6], params, (0.12, -0.03, 0.05), st[:2], int(st[2]),
            golden[f"{name}_m{m}_poses"], golden[f"{name}_m{m}_weights_in"], golden[f"{name}_m{m}_scan"], st[3])
    if nav.lib().navgpu_device_count() <= 0:
        with pytest.raises(subprocess.CalledProcessError) as e:
            B.run_update(*args)
        assert e.value.returncode == 3
        assert "navgpu status -2" in e.value.stderr and "no usable HIP device" in e.value.stderr
    else:
        upd, ws, wf, w, _, _, _ = B.run_update(*args)
        out = golden[f"{name}_m{m}_out"]
        assert upd == 1
        assert np.allclose(w, out[4:], rtol=1e-12, atol=0) and np.allclose([ws, wf], out[1:3], rtol=1e-12, atol=0)
