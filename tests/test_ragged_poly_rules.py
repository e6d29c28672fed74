"""The rules of the two-stage form on a clip table (python-soxr_amd/csrc/poly_rules.h ragged_poly_plan) on the CPU:
tests/c/ragged_poly_rules_check.cpp states each by brute force over a few thousand seeded tables — up and down, 1-3 channels,
float32 and float64, empty clips, clips one frame either side of the 8192-frame admission edge, columns above the byte budget,
more columns than one launch holds — and compares: every clip lands in exactly one class (empty, two-stage, short), by the
admission of the clip ALONE; each column's pad / n_core / n_mid equal two_stage_mid of that clip alone; the columns' extents
inside the intermediate are disjoint, 8-element aligned and inside the allocation; the rows of both stages describe exactly
those extents and the caller's columns, in both directions; the ranges respect both caps and cover every column once.
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


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_skip_comes_before_the_table_copy_and_the_first_barrier():
    """In k_poly<.., RAGGED> the skip test stands before the table is copied to LDS and before the first __syncthreads(): a
    workgroup behind its column's end must not leave a barrier half attended."""
    src = _read("twostage.hip")
    body = src[src.index("__global__ void __launch_bounds__(256) k_poly(typename PolyArgsOf<RAGGED>::type"):]
    skip = body.index("ragged_span_skip(")
    assert skip < body.index("tab[i] = g[i]") and skip < body.index("__syncthreads()")
    assert body.index("poly_column_args<Real>(") < skip, "the skip test reads the column's own n_out"
    # every tap count x MQ in {0, 1, -1} x {float, double} has a ragged instance: the one list that expands the equal-length ones
    pk = src[src.index("static void (*poly_kernel("):]
    pk = pk[:pk.index("HIPSOXR_POLY2_TAPS(")]
    assert "HIPSOXR_POLY_TAPS(HIPSOXR_POLY_T)" in pk and all(("k_poly<Real, t, %s, RAGGED>" % mq) in pk for mq in ("0", "1", "-1"))
    assert "poly_kernel<Real, true>(" in src, "launch_poly takes the ragged instance for a table"


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_brute_force(build, tmp_path):
    exe = str(tmp_path / ("ragged_poly_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "c", "ragged_poly_rules_check.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    print(ran.stdout[-3000:])
    assert ran.returncode == 0, ran.stdout[-3000:] + ran.stderr[-3000:]
    assert "checks, 0 failed" in ran.stdout
