"""The rules of k_fft_strided2 on a clip table (python-soxr_amd/csrc/fft_ragged_rules.h: the work-item map the kernel itself
walks, a clip's own item count, the grid of the longest clip, the conditions a table adds to the layout decision) on the
CPU: tests/c/fft_ragged_rules_check.cpp states each by brute force — over clip item counts {0, 1, 2, 7, 8, 9, 17} and
{1, 2, 3, 4} channel units the map visits every (clip, unit, item) below the clip's own count exactly once and nothing at
or above it (there is ONE source of per_xcd: the clip's own item count) — and compares.  It is a stand-alone program built
with the host compiler — once plain, once with the address and undefined-behaviour sanitizers — and run; nothing of it is
loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-soxr_amd", "csrc")

BUILDS = {
    "plain": ["-O1"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (g++, c++ or clang++)")


def test_header_needs_no_hip():
    """The rules compile and run on a CPU alone: the header includes the standard library, nothing of HIP or the engine."""
    with open(os.path.join(CSRC, "fft_ragged_rules.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert "<cstdint>" in includes
    assert not [i for i in includes if "hip" in i.lower() or i.startswith('"')], includes


def test_the_engine_uses_the_header():
    """the kernel walks the header's map; the layout decision and the row launcher ask its table conditions"""
    with open(os.path.join(CSRC, "fft.hip")) as f:
        src = f.read()
    assert '#include "fft_ragged_rules.h"' in src
    for fn in ("fft_xcd_map", "fft_plain_map", "fft_clip_items", "fft_xcd_grid_x", "fft_map_clips_ok", "fft_table_words_aligned", "fft_table_form_served"):
        assert fn + "(" in src, fn
    kernel = src[src.index("k_fft_strided2(FftArgs a)"):src.index("// Three translation units")]
    assert "fft_xcd_map(" in kernel and "fft_plain_map(" in kernel and "fft_clip_items(" in kernel, "the kernel itself calls the map"


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_brute_force(build, tmp_path):
    exe = str(tmp_path / ("fft_ragged_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "c", "fft_ragged_rules_check.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    print(ran.stdout[-3000:])
    assert ran.returncode == 0, ran.stdout[-3000:] + ran.stderr[-3000:]
    assert "checks, 0 failed" in ran.stdout
