"""CPU checks of the resampling yardstick: tests/golden/g10_amcl_resample.npz is what the reference amcl core (compiled in place)
computes, and the golden tool's drand48 replay is the documented 48-bit generator."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import amcl_reference_build as B  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g10_amcl_resample.npz")
needs_reference = pytest.mark.skipif(not B.available(), reason="the reference amcl tree is not on this machine")


@needs_reference
def test_resample_goldens_reproduce_from_the_reference(tmp_path):
    out = tmp_path / "g10.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_amcl_resample_goldens.py"), "--out", str(out)], check=True,
                   capture_output=True)
    new, old = np.load(out), np.load(GOLDEN)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert np.array_equal(old[k], new[k]), k


def test_drand48_replay_is_the_documented_generator():
    import make_amcl_resample_goldens as G
    g = G.Drand48(0)
    # srand48(0): state 0x330E; x1 = (0x5DEECE66D * 0x330E + 0xB) mod 2^48
    x1 = (0x5DEECE66D * 0x330E + 0xB) % (1 << 48)
    assert g() == x1 / float(1 << 48)


def test_golden_file_stays_small():
    assert os.path.getsize(GOLDEN) < 600 * 1024


def test_golden_cases_cover_the_issue_list():
    g = np.load(GOLDEN)
    names = {str(n) for n in g["cases"]}
    for model in ("multi", "sys"):
        for case in ("wdiff0_manybins", "kld_binds", "wdiff_pos", "one_bin", "min_clamp", "separated", "diagonal_pi", "converged",
                     "unconverged", "capped"):
            assert f"{model}_{case}" in names
    for name in names:
        out = g[name + "_out"]
        n = int(out[1])
        assert len(g[name + "_src"]) == n and len(g[name + "_pool"]) == int(out[7])
        assert len(g[name + "_clusters"]) == int(out[5])
    assert g["multi_one_bin_out"][1] == g["multi_one_bin_params"][2]          # one bin: the limit is max_samples
    assert g["multi_min_clamp_out"][1] == g["multi_min_clamp_params"][1] + 1   # the limit clamped to min_samples
    for model in ("multi", "sys"):                                             # the KLD limit binds below max_samples
        assert g[f"{model}_kld_binds_out"][1] < g[f"{model}_kld_binds_params"][2]
    assert g["sys_capped_out"][1] == g["sys_capped_params"][2]                 # new_count * (1 + w_diff) capped
    assert g["multi_converged_out"][6] == 1 and g["multi_unconverged_out"][6] == 0
    assert g["multi_diagonal_pi_out"][5] == 4                                    # diagonal touch joins; +-pi does not wrap
