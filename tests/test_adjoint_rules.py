"""The host rules of the transposed operator (python-soxr_amd/csrc/adjoint_rules.h: the transposed bank and the per-tile
tables, the launch form — lane-per-element or period-tiled kernel, lanes, LDS limit, channel groups, grid — and the two
entries' refusals) on the CPU: tests/c/adjoint_rules_check.cpp reads every coefficient of the tables back against the forward
bank through plan.h's locate(), holds the bounds adjoint.hip's REACH paragraph promises, computes the form of every case of
tests/test_gpu_adjoint_forms.py and compares with what the launch logs showed on the GPU, sweeps the form rule against its
properties and a transcription of the loops adj_launch had, and asks both entries' refusals over element type x selector x
plan kind x window x table x extents.  It is a stand-alone program built with the host compiler — once plain, once with the
address and undefined-behaviour sanitizers — and run; nothing of it is loaded into this process.  The rest of the module
reads source text: each rule stands in one place, and adjoint.hip's launch layer is a sequence of short functions."""
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
RULES = ("adj_tables", "adj_tile_form", "adj_gather_grid", "adj_interp_grid", "adj_entry_refusal", "adj_row_refusal", "adj_extent_refusal", "kAdjTooLong")
STEPS = ("adj_args", "adj_tile_form", "adj_launch_tile", "adj_launch_gather")


def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (g++, c++ or clang++)")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _code(text):
    """C++ text without its comments and string literals (an error text may say 65535; a rule may not)."""
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    return re.sub(r"//[^\n]*", "", text)


def _launch_layer():
    """adjoint.hip from adj_build to the end: tables, cache, launches, the two entries."""
    src = _read("adjoint.hip")
    return src[src.index("static const char *adj_build("):]


def _functions(text):
    """(name, lines) of every function defined at column 0, from its first line to its closing brace."""
    found = re.findall(r"(?<=\n)((?:template <[^\n]*>\n)?(?:[\w:<>]+[ \*&]+)+(\w+)\([^;{]*\)\n\{\n.*?\n\}\n)", "\n" + text, re.S)
    return [(name, body.count("\n")) for body, name in found]


def test_header_needs_no_hip():
    """The rules compile and run on a CPU alone: the header includes the standard library and job_rules.h, nothing of HIP or
    the engine, and reads no switch."""
    text = _read("adjoint_rules.h")
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert "<cstdint>" in includes
    assert [i for i in includes if i.startswith('"')] == ['"job_rules.h"'] and not [i for i in includes if "hip" in i.lower()], includes
    assert "__global__" not in text and "switches()" not in _code(text) and "getenv" not in text


def test_the_launch_layer_uses_the_header():
    """adjoint.hip decides through the header's functions: every rule is called, adj_launch is its three steps, and none of
    the numbers the header owns is written out in the launch layer."""
    src, layer = _read("adjoint.hip"), _launch_layer()
    assert '#include "adjoint_rules.h"' in src
    for name in RULES:
        assert re.search(r"\b" + name + r"\b", layer), name
    launch = layer[layer.index("static const char *adj_launch(const AdjBank"):]
    launch = launch[:launch.index("\n}\n")]
    for name in STEPS:
        assert name in launch, name
    code = _code(layer)
    for copy in (r"65535", r"2147483647", r"80\s*\*\s*1024", r"160\s*\*\s*1024", r"\b8192\b", r"\b65536\b"):
        assert not re.search(copy, code), "adjoint.hip's launch layer restates a rule of adjoint_rules.h: " + copy
    assert "floor_div(int64_t" not in src and "kAdjMinPeriods =" not in src and "kAdjRS =" not in src
    # one loop variable named rows is one too many beside the clip table's
    assert not re.search(r"\brows\s*=\s*\(", code)


def test_each_text_and_launch_stands_once():
    both = _read("adjoint_rules.h") + _read("adjoint.hip")
    assert both.count("too long for one launch") == 1
    for text in ("float32 or float64 elements only", "whole signals only", "the kernel selector must be AUTO or EXACT", "invalid job extent", '"null buffer"'):
        assert both.count(text) == 1, text
    sites = re.findall(r"hipLaunchKernelGGL\(\((k_adj_\w+)", _read("adjoint.hip"))
    assert sorted(sites) == ["k_adj_gather", "k_adj_interp", "k_adj_tile"], sites
    assert len(re.findall(r"HIPSOXR_F32 \?", _read("adjoint.hip"))) == 1  # with_real


def test_no_launch_function_is_long():
    """From adj_build to the end nothing is longer than 36 lines (the bar tests/test_job_rules.py holds for the dispatcher)."""
    sizes = _functions(_launch_layer())
    names = {n for n, _ in sizes}
    assert {"adj_build", "adj_ensure", "adj_launch_log", "adj_interp_log", "adj_args", "adj_launch_tile", "adj_launch_gather", "adj_launch", "adj_interp_launch",
            "launch_adjoint", "launch_adjoint_ragged"} <= names, names
    for name, lines in sizes:
        assert lines <= 36, (name, lines)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_slow_statements(build, tmp_path):
    exe = str(tmp_path / ("adjoint_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC,
           os.path.join(ROOT, "tests", "c", "adjoint_rules_check.cpp"), os.path.join(CSRC, "plan.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    print(ran.stdout[-3000:])
    assert ran.returncode == 0, ran.stdout[-3000:] + ran.stderr[-3000:]
    assert re.search(r"\b[1-9]\d* checks, 0 failed", ran.stdout)
