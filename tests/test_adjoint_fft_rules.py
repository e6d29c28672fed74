"""The host rules of the adjoint on the frequency-domain engine (python-soxr_amd/csrc/adjoint_fft_rules.h: the transposed
plan's tap count and bank, the selector's ordered refusal list) on the CPU: tests/c/adjoint_fft_rules_check.cpp reads every
entry of the transposed bank back against the forward bank through plan.h's locate() and meets every forward coefficient
exactly once, holds T' to a multiple of 8 that cannot lose 8, compares Im H of the transposed plan with the forward plan's by
one and the same code (both figures printed), and sweeps the refusals over element type x selector x plan kind x window x
table — for the HQ / VHQ rate pairs of tests/test_gpu_adjoint.py and every (L, M) of fft.hip's fft_pairs.  It is a stand-alone
program built with the host compiler — once plain, once with the address and undefined-behaviour sanitizers — and run;
nothing of it is loaded into this process.  The rest of the module reads source text."""
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
    text = _read("adjoint_fft_rules.h")
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert sorted(i for i in includes if i.startswith('"')) == ['"job_rules.h"', '"plan.h"'], includes
    assert not [i for i in includes if "hip" in i.lower()]
    assert "__global__" not in text and "switches()" not in _code(text) and "getenv" not in text


def test_each_text_stands_once_and_the_entries_branch_once():
    rules, unit, adjoint = _read("adjoint_fft_rules.h"), _read("adjoint_fft.hip"), _read("adjoint.hip")
    texts = re.findall(r'"(adjoint job: HIPSOXR_KERNEL_ADJOINT_FFT[^"]*)"', rules)
    assert len(texts) == 9 and len(set(texts)) == 9, texts  # eight refusals and the engine's "unavailable"
    everything = rules + unit + adjoint + _read("engine.cpp")
    for t in texts:
        assert everything.count(t) == 1, t
    assert everything.count("HIPSOXR_KERNEL_ADJOINT_FFT selects the transposed operator") == 1
    # one early branch per entry, nothing else of the selector in adjoint.hip; no kernel and no launch in the new unit
    assert len(re.findall(r"j\.kernel == HIPSOXR_KERNEL_ADJOINT_FFT\) return launch_adjoint_fft(?:_ragged)?\(p, j, stream\);", adjoint)) == 2
    assert _code(adjoint).count("HIPSOXR_KERNEL_ADJOINT_FFT") == 2
    assert "__global__" not in unit and "hipLaunchKernelGGL" not in unit
    assert "launch_fft(pt, f, stream, &handled)" in unit and "fft_job_eligible" not in _code(unit)
    assert "adjoint_fft_release(p)" in adjoint[adjoint.index("void adjoint_release("):adjoint.index("template <typename Real>\nstatic const char *adj_upload")]
    with open(os.path.join(ROOT, "python-soxr_amd", "build.sh")) as f:
        assert f.read().count("adjoint_fft.o") == 2  # compiled, linked


def test_the_restated_table_is_the_engine_s():
    """tests/c/adjoint_fft_rules_check.cpp sweeps a restatement of fft_pairs' full-size rows: held to fft.hip here."""
    rows = set()
    for L, M, k, small in re.findall(r"HIPSOXR_PAIR\((\d+), (\d+), (\d+), (\w+),", _read("fft.hip")):
        if small == "false":
            rows.add((int(L), int(M), int(k)))
    with open(os.path.join(ROOT, "tests", "c", "adjoint_fft_rules_check.cpp")) as f:
        text = f.read()
    body = text[text.index("kRows[] = {"):text.index("static int row_k")]
    restated = {tuple(int(v) for v in m) for m in re.findall(r"\{(\d+), (\d+), (\d+)\}", body)}
    assert restated == rows and len(rows) == 30, (restated ^ rows)
    every = {(int(L), int(M)) for L, M in re.findall(r"HIPSOXR_PAIR(?:_F32)?\((\d+), (\d+),", _read("fft.hip"))}
    assert every == {(L, M) for L, M, _ in rows}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_slow_statements(build, tmp_path):
    exe = str(tmp_path / ("adjoint_fft_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC,
           os.path.join(ROOT, "tests", "c", "adjoint_fft_rules_check.cpp"), os.path.join(CSRC, "plan.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    print(ran.stdout[-6000:])
    assert ran.returncode == 0, ran.stdout[-3000:] + ran.stderr[-3000:]
    assert re.search(r"\b[1-9]\d* checks, 0 failed", ran.stdout)
    assert ran.stdout.count("Im H / max Re H: forward") == 7 + 2 * 30
