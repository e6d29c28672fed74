"""The integer rules of a ragged exact launch (python-soxr_amd/csrc/ragged_rules.h: grid size from the longest clip, the skip
test, the total-slab count, the 65535-column fold) on the CPU: tests/c/ragged_rules_check.cpp states each by brute force over
random tables and geometries and compares — a block is skipped exactly when no output of its clip lies in it, the blocks kept
cover [0, out_frames) of every clip, the folded ranges partition the clips.  It is a stand-alone program built with the host
compiler — once plain, once with the address and undefined-behaviour sanitizers — and run; nothing of it is loaded into this
process."""
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
    """The rules compile and run on a CPU alone: the header includes the standard library, nothing of HIP or the engine — and
    job_rules.h, whose constants it shares and which tests/test_job_rules.py holds to the same."""
    with open(os.path.join(CSRC, "ragged_rules.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert "<cstdint>" in includes
    assert not [i for i in includes if "hip" in i.lower() or (i.startswith('"') and i != '"job_rules.h"')], includes


def test_the_launcher_and_the_kernels_use_the_header():
    """kernels.hip sizes its ragged grids and folds its tables through the header's functions, not through copies."""
    with open(os.path.join(CSRC, "kernels.hip")) as f:
        src = f.read()
    assert '#include "ragged_rules.h"' in src
    for name in ("ragged_longest", "ragged_grid_x", "ragged_total_slabs", "ragged_gather_grid_x", "ragged_fold_range"):
        assert name + "(" in src, name


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_brute_force(build, tmp_path):
    exe = str(tmp_path / ("ragged_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "c", "ragged_rules_check.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    print(ran.stdout[-3000:])
    assert ran.returncode == 0, ran.stdout[-3000:] + ran.stderr[-3000:]
    assert "checks, 0 failed" in ran.stdout
