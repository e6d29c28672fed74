"""The rules of HIPSOXR_KERNEL_ADJOINT_AUTO (python-soxr_amd/csrc/adjoint_auto_rules.h: the selector's refusals, the engine the
transpose of AUTO's forward runs on, the cut of a clip table for the transposed two-stage form) on the CPU:
tests/c/adjoint_auto_rules_check.cpp sweeps the decision table over plan kind x recipe x 8191 / 8192 total outputs x switches x
form x admits x entry, the refusals over both entries, and checks the partition, the compacted short sub-table, every
two-stage column's poly row and transposed FFT row against what the equal-length launcher sets for the clip alone, and the
ranges, over seeded random adjoint tables.  It is a stand-alone program built with the host compiler — once plain, once with
the address and undefined-behaviour sanitizers — and run; nothing of it is loaded into this process.  The rest of the module
reads source text: the selector's texts stand once, in the header; adjoint.hip and engine.cpp only hand over; the launchers'
inner functions are called, not copied."""
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


def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (g++, c++ or clang++)")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _code(text):
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    return re.sub(r"//[^\n]*", "", text)


def test_header_needs_no_hip():
    text = _read("adjoint_auto_rules.h")
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert sorted(i for i in includes if i.startswith('"')) == ['"job_rules.h"', '"poly_adj_rules.h"'], includes
    assert not [i for i in includes if "hip" in i.lower()]
    assert "__global__" not in text and "switches()" not in _code(text) and "getenv" not in text


def test_each_text_stands_once_and_the_entries_hand_over():
    rules, unit, adjoint, engine, two = (_read(n) for n in ("adjoint_auto_rules.h", "adjoint_auto.hip", "adjoint.hip", "engine.cpp", "twostage.hip"))
    texts = re.findall(r'"((?:adjoint job: )?HIPSOXR_KERNEL_ADJOINT_AUTO[^"]*)"', rules)
    assert len(texts) == 12 and len(set(texts)) == 12, texts  # six refusals, the forward entry, the late decline, four table failures
    everything = rules + unit + adjoint + engine + two + _read("adjoint_fft.hip")
    for t in texts:
        assert everything.count(t) == 1, t
    for src in (unit, adjoint, engine, two):  # no text of the selector outside the header
        assert not re.findall(r'"[^"\n]*HIPSOXR_KERNEL_ADJOINT_AUTO[^"\n]*"', src)
    # one line per entry in adjoint.hip, one in engine.cpp
    assert len(re.findall(r"j\.kernel == HIPSOXR_KERNEL_ADJOINT_AUTO\) return launch_adjoint_auto(?:_ragged)?\(p, j, stream\);", adjoint)) == 2
    assert _code(adjoint).count("HIPSOXR_KERNEL_ADJOINT_AUTO") == 2 and _code(engine).count("HIPSOXR_KERNEL_ADJOINT_AUTO") == 1
    assert "job->kernel == HIPSOXR_KERNEL_ADJOINT_AUTO) return kAdjAutoForwardRefusal;" in engine
    # the new unit decides through the header and launches nothing itself
    assert "__global__" not in unit and "hipLaunchKernelGGL" not in unit
    for name in ("adj_auto_refusal", "adj_auto_engine", "adj_auto_total_equal", "adj_auto_total_table", "adj_fft_try", "launch_adjoint_two_stage_try",
                 "launch_adjoint_two_stage_ragged", "adj_exact_run", "adj_row_refusal", "adj_extent_refusal"):
        assert re.search(r"\b" + name + r"\b", _code(unit)), name
    # ... and the ragged launcher through ragged_poly_adj_plan, which wraps ragged_poly_plan's body (one definition)
    assert "ragged_poly_adj_plan(" in _code(two) and _read("poly_rules.h").count("g.count == kPolyMaxCols ||") == 1
    assert "ragged_poly_plan_by(" in _code(rules)
    with open(os.path.join(ROOT, "python-soxr_amd", "build.sh")) as f:
        assert f.read().count("adjoint_auto.o") == 2  # compiled, linked


def test_the_inner_functions_are_shared_not_copied():
    fft, two, adjoint = _read("adjoint_fft.hip"), _read("twostage.hip"), _read("adjoint.hip")
    # one call of launch_fft on the transposed plan; the named selector is the handled / not-handled form plus its error
    assert fft.count("launch_fft(pt, f, stream, &handled)") == 1 and "adj_fft_try(p, j, stream, rows, &handled)" in fft
    # one admission and one pair of launches for the equal-length transposed form
    assert _code(two).count("two_stage_adj_run(") == 2 and "launch_adjoint_two_stage_try(p, j, stream, &handled)" in two
    # the ragged kernel is a second instantiation of the same template, launched on its own line
    assert "template <typename Real, int TT, bool RAGGED = false>\n__global__ void __launch_bounds__(256) k_poly_adj(typename PolyArgsOf<RAGGED>::type a_)" in two
    assert len(re.findall(r"hipLaunchKernelGGL\(kern_r, grid, dim3\(256\), lds, st, ar\);", two[two.index("launch_poly_adj("):two.index("run_poly_adj(")])) == 1
    # the exact adjoint: adj_run behind one exposed function
    assert _code(adjoint).count("adj_run(*p, b, j,") == 3


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_slow_statements(build, tmp_path):
    exe = str(tmp_path / ("adjoint_auto_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC,
           os.path.join(ROOT, "tests", "c", "adjoint_auto_rules_check.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    print(ran.stdout[-3000:])
    assert ran.returncode == 0, ran.stdout[-3000:] + ran.stderr[-3000:]
    assert re.search(r"\b[1-9]\d* checks, 0 failed", ran.stdout)
    assert re.search(r"decision table: 512 cases, [1-9]\d* on the frequency-domain engine, [1-9]\d* on the two-stage form", ran.stdout)
