"""The integer rules of a ragged launch on an interpolated-phase plan (python-soxr_amd/csrc/ragged_rules.h: the frame-axis grid
of "U outputs of one column per workgroup" from the longest clip, the skip test, the count of workgroups that do work) on the
CPU: tests/c/ragged_interp_rules_check.cpp states each by brute force over random tables and U and compares — a workgroup is
skipped exactly when no output of its clip lies in it, the workgroups kept cover [0, out_frames) of every clip once, the total
equals the count.  It is a stand-alone program built with the host compiler — once plain, once with the address and
undefined-behaviour sanitizers — and run; nothing of it is loaded into this process."""
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


def test_the_launcher_and_the_kernels_use_the_rules():
    """kernels.hip sizes the ragged grids of the interpolated kernels and feeds their cost model through the header's
    functions; the kernels ask the header's skip tests."""
    with open(os.path.join(CSRC, "kernels.hip")) as f:
        src = f.read()
    for name in ("ragged_span_grid_x", "ragged_span_total", "ragged_total_out", "ragged_gather_grid_x", "ragged_fold_range"):
        assert name + "(" in src, name
    with open(os.path.join(CSRC, "kernels_interp.h")) as f:
        ksrc = f.read()
    assert ksrc.count("ragged_span_skip(") == 2 and ksrc.count("ragged_gather_skip(") == 1


def test_skip_comes_before_the_first_barrier_and_before_any_position():
    """In k_interp_wave and k_interp_tile the skip test stands before the first __syncthreads() and the first interp_locate:
    a workgroup behind its clip's end (every workgroup of an empty clip) must neither locate output -1 nor leave a barrier
    half attended."""
    with open(os.path.join(CSRC, "kernels_interp.h")) as f:
        ksrc = f.read()
    for kernel in ("k_interp_wave(typename", "k_interp_tile(typename"):
        body = ksrc[ksrc.index(kernel):]
        skip = body.index("ragged_span_skip(")
        assert skip < body.index("__syncthreads()"), kernel
        assert skip < body.index("interp_locate<"), kernel


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_brute_force(build, tmp_path):
    exe = str(tmp_path / ("ragged_interp_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "c", "ragged_interp_rules_check.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    print(ran.stdout[-3000:])
    assert ran.returncode == 0, ran.stdout[-3000:] + ran.stderr[-3000:]
    assert "checks, 0 failed" in ran.stdout
