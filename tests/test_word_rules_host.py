"""k_merge's word forms (navigation_amd/csrc/costmap_word_rules.h) against the plain per-byte rules, on the CPU: tools/word_rules_check.cpp
is built with the host compiler - with the undefined-behaviour and address sanitizers where the compiler has them - and run.
It covers all 65 536 (static, obstacle) byte pairs (old master, obstacle for the layer-only merge), every old master byte, the four byte
positions and the sixteen in-box masks of a word for every setting of the kernel, the group bitmaps, and the division by multiplication."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_word_rules_against_byte_rules(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "word_rules_check")
    base = [cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "navigation_amd", "csrc"), os.path.join(ROOT, "tools", "word_rules_check.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if san.returncode != 0:  # a compiler without the sanitizer runtimes: the comparison itself still runs
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, plain.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 15 and all(" ok (0)" in ln for ln in lines), run.stdout
