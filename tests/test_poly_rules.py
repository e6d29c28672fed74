"""The rules of the two-stage form's polyphase launch (python-soxr_amd/csrc/poly_rules.h: kernel form, tile size in LDS, run
length, lane order, grid, admission, intermediate layout) on the CPU: tests/c/poly_rules_check.cpp states each slowly and
independently over random stages and jobs and over real stages, and compares — every tile's source span within span_max by
the kernels' own 64.64 positions and by exact ones, an admitted job's tile within 160 KiB, the lane multiplier an odd
bijection whose conflict cost equals a plain recount and which no smaller multiplier beats, a split column's segments a whole
number of periods apart, column groups that divide the channel count, the grid rule, the intermediate signal's pad and
strides.  It is a stand-alone program built with the host compiler — once plain, once with the address and
undefined-behaviour sanitizers — and run; nothing of it is loaded into this process."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-soxr_amd", "csrc")

BUILDS = {
    "plain": ["-O1"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
RULES = ("poly_stage", "poly_form", "poly_cols", "poly_span_max", "poly_lds_bytes", "poly_rmax", "poly_occ_limit", "poly_slots", "poly_lane_cost",
         "poly_pick_run", "poly_tiles", "poly_grid_x", "poly_step_fx", "poly_fx_per_rem", "two_stage_admits", "two_stage_mid")


def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (g++, c++ or clang++)")


def test_header_needs_no_hip():
    """The rules compile and run on a CPU alone: the header includes the standard library, nothing of HIP or the engine."""
    with open(os.path.join(CSRC, "poly_rules.h")) as f:
        text = f.read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert "<cstdint>" in includes
    assert not [i for i in includes if "hip" in i.lower() or i.startswith('"')], includes
    assert "__global__" not in text and "__device__" not in text


def test_the_launcher_uses_the_header():
    """twostage.hip decides through the header's functions, not through copies: every rule is called, and none of the
    expressions the header owns is written out in the launcher's host code."""
    with open(os.path.join(CSRC, "twostage.hip")) as f:
        src = f.read()
    assert '#include "poly_rules.h"' in src
    for name in RULES:
        assert name + "(" in src, name
    host = src[src.index("static PolyArgs poly_args("):]     # the launch layer: behind the kernels
    assert "__global__" not in host
    for copy in (r"257", r"160\s*\*\s*1024", r"150u?\s*\*\s*1024", r"65535", r"&=\s*~7u", r"12\.\s*\*\s*256", r"\.02\s*\*", r"8192"):
        assert not re.search(copy, host), "twostage.hip's launch layer restates a rule of poly_rules.h: " + copy
    # the instance lists expand in one function of the launch layer
    assert host.count("HIPSOXR_POLY_TAPS(") == 1 and host.count("HIPSOXR_POLY2_TAPS(") == 1
    assert host.index("poly_kernel(") < host.index("HIPSOXR_POLY_TAPS(") < host.index("HIPSOXR_POLY2_TAPS(") < host.index("poly_trace_begin")


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_slow_statements(build, tmp_path):
    exe = str(tmp_path / ("poly_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "c", "poly_rules_check.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    print(ran.stdout[-3000:])
    assert ran.returncode == 0, ran.stdout[-3000:] + ran.stderr[-3000:]
    assert re.search(r"\b[1-9]\d* checks, 0 failed", ran.stdout)
