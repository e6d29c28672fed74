"""The stream layer's pure rules (python-soxr_amd/csrc/stream_rules.h: k_avail, ring_keep, ring_grow, emit_count, the
variable-rate clock) on the CPU: tests/c/stream_rules_check.cpp holds a slow, independent statement of each and compares.
It is a stand-alone program built with the host compiler — once plain, once with the address and undefined-behaviour
sanitizers — and run; nothing of it is loaded into this process."""
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
    """The rules compile and run on a CPU alone: the header includes plan.h and the standard library, nothing of HIP."""
    with open(os.path.join(CSRC, "stream_rules.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert '"plan.h"' in includes and "<cstdint>" in includes
    assert not [i for i in includes if "hip" in i.lower() or i == '"device.h"'], includes


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_their_slow_statements(build, tmp_path):
    exe = str(tmp_path / ("stream_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC,
           os.path.join(ROOT, "tests", "c", "stream_rules_check.cpp"), os.path.join(CSRC, "plan.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    print(ran.stdout[-3000:])
    assert ran.returncode == 0, ran.stdout[-3000:] + ran.stderr[-3000:]
    assert "checks, 0 failed" in ran.stdout
