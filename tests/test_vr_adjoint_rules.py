"""The rules of the ragged variable-rate adjoint (python-soxr_amd/csrc/vr_adjoint_rules.h: the range of cotangent samples a
gradient frame sums over, the grid, what is refused of a row) on the CPU.  tests/c/vr_adjoint_rules_check.cpp compares the
range rule — a double-precision estimate corrected with exact 128-bit products, what the kernel itself calls — with a true
128-bit division and with its defining property; it is a stand-alone program built with the host compiler — once plain, once
with the address and undefined-behaviour sanitizers — and run; nothing of it is loaded into this process.  Every
(a, H, S, n_y, k_lo, k_hi) it evaluated is printed, recomputed here in exact Python integers and checked by brute force over
k: k is in the range iff (a - H) 2^64 <= k S < (a + H) 2^64 and 0 <= k < n_y."""
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "python-soxr_amd", "csrc")
sys.path.insert(0, HERE)
from vr_sim import ONE, q64  # noqa: E402

BUILDS = {
    "plain": ["-O1"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
RATIOS = (2.0 ** -19, 0.5, 0.9070294784580499, 1.0, 1.1, 1.1 * (1 - 2.0 ** -40), 3.0, 2.0 ** 19)
BRUTE = 4096  # ranges up to this many samples are walked whole, with a margin either side; longer ones at both ends


def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (g++, c++ or clang++)")


def _member(k, a, H, S, n_y):
    return 0 <= k < n_y and (a - H) * ONE <= k * S < (a + H) * ONE


def test_header_needs_no_hip():
    with open(os.path.join(CSRC, "vr_adjoint_rules.h")) as f:
        text = f.read()
    includes = [line.split()[1] for line in text.split("\n") if line.startswith("#include")]
    assert '"vr_ragged_rules.h"' in includes and '"adjoint_rules.h"' in includes
    assert not [i for i in includes if "hip" in i.lower() or i == '"device.h"'], includes


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_range_rule_in_exact_integers_and_by_brute_force(build, tmp_path):
    exe = str(tmp_path / ("vr_adjoint_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "vr_adjoint_rules_check.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    tail = "\n".join(ln for ln in ran.stdout.split("\n") if not ln.startswith("RANGE "))
    print(tail[-3000:])
    assert ran.returncode == 0, tail[-3000:] + ran.stderr[-3000:]
    assert "checks, 0 failed" in ran.stdout
    rows = [tuple(int(v) for v in ln.split()[1:]) for ln in ran.stdout.split("\n") if ln.startswith("RANGE ")]
    assert len(rows) >= 8 * 2 * 12 * 6 + 4000
    assert {q64(r) for r in RATIOS} <= {(hi << 64) | lo for _, _, hi, lo, _, _, _ in rows}, "the issue's eight ratios, as q64 truncates them"
    frames = {a for a, H, _, _, _, _, _ in rows if H == 108}
    assert {0, 107, 108, 109, 255, 256, 257, 2 ** 31 - 1, 2 ** 31} <= frames
    assert {0, 1} <= {n for _, _, _, _, n, _, _ in rows}
    cut_inside = walked = 0
    for a, H, hi, lo, n_y, k_lo, k_hi in rows:
        S = (hi << 64) | lo
        want_lo = max(0, -((-(a - H) * ONE) // S))
        ceil_hi = -((-(a + H) * ONE) // S)
        assert (k_lo, k_hi) == (want_lo, min(n_y, ceil_hi) - 1), (a, H, S, n_y, k_lo, k_hi)
        cut_inside += want_lo < n_y < ceil_hi
        # brute force over k: every sample of the range is a member, none of its surroundings is (membership is an interval
        # in k — k S is increasing — so a long range is decided by its ends)
        if k_hi - k_lo < BRUTE:
            ks = range(max(0, k_lo - 64), k_hi + 65)
            walked += 1
        else:
            ks = list(range(max(0, k_lo - 64), k_lo + 64)) + list(range(k_hi - 64, k_hi + 65))
        for k in ks:
            assert _member(k, a, H, S, n_y) == (k_lo <= k <= k_hi), (a, H, S, n_y, k_lo, k_hi, k)
        if k_lo > k_hi:  # an empty range: no sample of the cotangent at all is a member — its last one, and the first one
            # at or behind the window's start, decide that
            assert not _member(n_y - 1, a, H, S, n_y) and not _member(min(want_lo, max(n_y - 1, 0)), a, H, S, n_y)
    assert cut_inside >= 100 and walked >= 2000
