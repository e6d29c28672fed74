"""The rules of a ragged variable-rate launch (python-soxr_amd/csrc/vr_ragged_rules.h: vr_const_out_len, the table's largest
step, what is refused of a ratio and a row) on the CPU.  tests/c/vr_ragged_rules_check.cpp compares the closed form with the
stream layer's own limit (stream_rules.h vr_k_limit on a constant-step clock) and the other rules with tables written by
hand; it is a stand-alone program built with the host compiler — once plain, once with the address and undefined-behaviour
sanitizers — and run; nothing of it is loaded into this process.  Every (n_in, step, count) it compared is printed, and
checked here once more against tests/vr_sim.py's VrSim._limit(True) in exact Python integers."""
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "python-soxr_amd", "csrc")
sys.path.insert(0, HERE)
from vr_sim import ONE, VrSim, q64  # noqa: E402

BUILDS = {
    "plain": ["-O1"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
RATIOS = (2.0 ** -19, 0.5, 0.9070294784580499, 1.0, 1.1, 1.1 * (1 - 2.0 ** -40), 3.0, 2.0 ** 19)


def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (g++, c++ or clang++)")


def _sim_limit(n_in, step):
    """VrSim's end-of-input limit for n_in frames on a fresh clock of constant step `step` (no oracle, no signal: the
    limit reads the input's length alone)"""
    sim = VrSim.__new__(VrSim)
    sim.k_s = sim.n_slew = sim.t_s = sim.delta = sim.k_done = 0
    sim.s0 = sim.s1 = step
    sim.H = 0  # (not read at end of input)
    sim.x = range(n_in)
    return sim._limit(True)


def test_header_needs_no_hip():
    with open(os.path.join(CSRC, "vr_ragged_rules.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert '"stream_rules.h"' in includes and '"ragged_rules.h"' in includes
    assert not [i for i in includes if "hip" in i.lower() or i == '"device.h"'], includes


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_the_stream_layer_and_the_simulator(build, tmp_path):
    exe = str(tmp_path / ("vr_ragged_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC,
           os.path.join(ROOT, "tests", "c", "vr_ragged_rules_check.cpp"), os.path.join(CSRC, "plan.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    tail = "\n".join(ln for ln in ran.stdout.split("\n") if not ln.startswith("LEN "))
    print(tail[-3000:])
    assert ran.returncode == 0, tail[-3000:] + ran.stderr[-3000:]
    assert "checks, 0 failed" in ran.stdout
    rows = [tuple(int(v) for v in ln.split()[1:]) for ln in ran.stdout.split("\n") if ln.startswith("LEN ")]
    assert len(rows) >= 7 * 8 + 4000
    steps = {(hi << 64) | lo for _, hi, lo, _ in rows}
    assert {q64(r) for r in RATIOS} <= steps, "the issue's eight ratios, as set_io_ratio truncates them"
    lens = {n for n, _, _, _ in rows[:56]}
    assert {0, 1, 1000, 2 ** 31 + 7} <= lens and len(lens) == 7
    for n_in, hi, lo, count in rows:
        step = (hi << 64) | lo
        assert count == _sim_limit(n_in, step), (n_in, step, count)
        if n_in == 0:
            assert count == 0
        if count:  # the closed form's own statement: the last output's half step still lies inside the input, the next one's not
            assert (count - 1) * step + step // 2 <= n_in * ONE < count * step + step // 2
