"""The rules of a float16 / bfloat16 device job (python-soxr_amd/csrc/half_rules.h: fused or not, the float32 temporaries'
strides, bytes and ranges, the copy kernels' index walk) on the CPU: tests/c/half_rules_check.cpp states each by brute force
over a grid of stride orders, shapes and byte limits and compares — the strides address every element exactly once in the
caller's dimension order, the ranges cover every (clip, channel) once within the limit, the fused decision agrees with its
restatement.  It is a stand-alone program built with the host compiler — once plain, once with the address and
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


def test_header_needs_no_hip():
    """The rules compile and run on a CPU alone: the header includes the standard library, nothing of HIP or the engine — and
    job_rules.h, whose constants it shares and which tests/test_job_rules.py holds to the same."""
    with open(os.path.join(CSRC, "half_rules.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert "<cstdint>" in includes
    assert not [i for i in includes if "hip" in i.lower() or (i.startswith('"') and i != '"job_rules.h"')], includes


def test_the_launchers_use_the_header():
    """launch_job, the frequency-domain engine's row launcher and the widening pass decide through the header's functions."""
    uses = {"kernels.hip": ("half_try_fused",), "fft.hip": ("half_fused_form",),
            "half.hip": ("half_pack", "half_cut", "half_range", "half_unpack")}
    for name, fns in uses.items():
        with open(os.path.join(CSRC, name)) as f:
            src = f.read()
        assert '#include "half_rules.h"' in src, name
        for fn in fns:
            assert fn + "(" in src, (name, fn)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_brute_force(build, tmp_path):
    exe = str(tmp_path / ("half_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "c", "half_rules_check.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    print(ran.stdout[-3000:])
    assert ran.returncode == 0, ran.stdout[-3000:] + ran.stderr[-3000:]
    assert "checks, 0 failed" in ran.stdout
