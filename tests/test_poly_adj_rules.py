"""The rules of the two-stage form's adjoint (python-soxr_amd/csrc/poly_adj_rules.h: the bracket of outputs that can reach a
run of samples, the tile and its LDS bytes, the grid, admission, the selector's refusals) on the CPU:
tests/c/poly_adj_rules_check.cpp enumerates every output k near a tile with its position taken both ways — the exact rational
and the kernels' truncated 64.64 step — and holds that no contributing k falls outside the bracket or outside a thread's
staged-index range, that the span bound covers every tile, that an admitted job's tile fits LDS, and that the transposed
plans of FFT-stage-shaped banks read back entry for entry through plan.h's locate().  It is a stand-alone program built with
the host compiler — once plain, once with the address and undefined-behaviour sanitizers — and run; nothing of it is loaded
into this process.  The rest of the module reads source text."""
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
RULES = ("poly_adj_run", "poly_adj_tile", "poly_adj_span_max", "poly_adj_lds_bytes", "poly_adj_tiles", "poly_adj_grid_x", "poly_adj_admits",
         "poly_adj_bracket", "poly_adj_run_span", "poly_adj_refusal", "kPolyAdjUnavailable")


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
    text = _read("poly_adj_rules.h")
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert [i for i in includes if i.startswith('"')] == ['"poly_rules.h"'] and not [i for i in includes if "hip" in i.lower()], includes
    assert "__global__" not in text and "switches()" not in _code(text) and "getenv" not in text


def test_the_launcher_uses_the_header():
    """twostage.hip decides through the header's functions; each text of the selector stands once, in the header; adjoint.hip
    and engine.cpp only hand over."""
    src, rules, adjoint, engine = _read("twostage.hip"), _read("poly_adj_rules.h"), _read("adjoint.hip"), _read("engine.cpp")
    assert '#include "poly_adj_rules.h"' in src
    for name in RULES:
        assert re.search(r"\b" + name + r"\b", src), name
    texts = re.findall(r'"((?:adjoint job: )?HIPSOXR_KERNEL_ADJOINT_TWO_STAGE[^"]*)"', rules)
    assert len(texts) == 8 and len(set(texts)) == 8, texts  # five refusals, the ragged entry, "unavailable", the forward entry
    everything = src + rules + adjoint + engine + _read("adjoint_fft.hip")
    for t in texts:
        assert everything.count(t) == 1, t
    assert len(re.findall(r"j\.kernel == HIPSOXR_KERNEL_ADJOINT_TWO_STAGE\) return ", adjoint)) == 2
    assert _code(adjoint).count("HIPSOXR_KERNEL_ADJOINT_TWO_STAGE") == 2 and _code(engine).count("HIPSOXR_KERNEL_ADJOINT_TWO_STAGE") == 1
    # the kernel shares the forward's position arithmetic: one definition, used by both
    assert src.count("struct PolyPosFx") == 1 and src.count("const PolyPosFx position{") == 3
    assert src.count("__umul64hi(dk, a.step_fx)") == 1
    # the transposed plan is built by adjoint_fft.hip's function, not copied
    assert "adj_fft_transposed(ts->fft)" in src and "adj_fft_bank" not in _code(src)
    # one launch site, no atomics
    assert len(re.findall(r"hipLaunchKernelGGL\(kern, grid, dim3\(256\), lds, st, a\);", src[src.index("launch_poly_adj("):])) == 1
    kernel = src[src.index("__global__ void __launch_bounds__(256) k_poly_adj"):src.index("// k_poly_adj's instances")]
    assert "atomic" not in kernel.lower()


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_brute_force(build, tmp_path):
    exe = str(tmp_path / ("poly_adj_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC,
           os.path.join(ROOT, "tests", "c", "poly_adj_rules_check.cpp"), os.path.join(CSRC, "plan.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    print(ran.stdout[-3000:])
    assert ran.returncode == 0, ran.stdout[-3000:] + ran.stderr[-3000:]
    assert re.search(r"\b[1-9]\d* checks, 0 failed", ran.stdout)
    assert re.search(r"\b[1-9]\d* positions one sample lower by the truncated step", ran.stdout)
    assert ran.stdout.count("coefficients each met once") == 5
