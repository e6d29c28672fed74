"""The rules of the device-job dispatcher (python-soxr_amd/csrc/job_rules.h: the refusals made before the device is asked for
anything, the engine order — frequency-domain engine, two-stage form, exact engine — and its AUTO threshold, the clip-row
check in both directions, the 65535-column fold) on the CPU: tests/c/job_rules_check.cpp states each slowly and independently
and compares — the fold's ranges against a transcription of the loops launch_job had, every column once and no range above
65535 columns, for counts up to 2^32 - 1; the row check against brute force; the engine truth table written on the raw
selector values; job_wide_lane at its edges; a table and an equal-length job of equal totals.  It is a stand-alone program built
with the host compiler — once plain, once with the address and undefined-behaviour sanitizers — and run; nothing of it is
loaded into this process.  The rest of the module reads source text: each rule stands in one place."""
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
DISPATCH = ("job_entry_refusal", "launch_job_table", "launch_job_half", "launch_job_folded", "launch_job_engines", "with_elem")
RULES = ("job_empty", "job_resident_refusal", "job_pcm_refusal", "job_half_refusal", "job_table_refusal", "job_fft_stream_refusal", "job_row_check", "job_try_fft",
         "job_two_stage_table", "job_two_stage", "job_wide_lane", "job_fold", "job_fold_range")


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


def _function(src, head):
    """The text of the function whose definition starts with `head` (up to the closing brace in column 0)."""
    a = src.index(head)
    return src[a:src.index("\n}\n", a) + 3]


def _launch_layer():
    """kernels.hip from the clip table's device copy to the end: the launches over a clip table, the many-streams launch and
    the dispatcher, with the host halves of the resident mailbox and the copy kernels between them."""
    src = _read("kernels.hip")
    return src[src.index("const char *clip_table_device("):]


def test_header_needs_no_hip():
    """The rules compile and run on a CPU alone: the header includes the standard library, nothing of HIP or the engine, and
    reads no switch but through its arguments."""
    text = _read("job_rules.h")
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert "<cstdint>" in includes
    assert not [i for i in includes if "hip" in i.lower() or i.startswith('"')], includes
    assert "__global__" not in text and "__device__" not in text
    assert "switches()" not in _code(text)


def test_the_dispatcher_uses_the_header():
    """kernels.hip decides through the header's functions, not through copies: every rule is called, and none of the numbers
    the header owns is written out in the launch layer."""
    layer = _launch_layer()
    assert '#include "job_rules.h"' in _read("kernels.hip") and '#include "job_rules.h"' in _read("adjoint.hip")
    for name in RULES:
        assert name + "(" in layer, name
    for name in DISPATCH:
        assert name + "(" in _function(layer, "\nconst char *launch_job("), name
    code = _code(layer)
    for copy in (r"65535", r"1\s*<<\s*13", r"\b8192\b", r"4\s*\*\s*\(size_t\)"):
        assert not re.search(copy, code), "kernels.hip's launch layer restates a rule of job_rules.h: " + copy
    assert not re.search(r"4\s*\*\s*\(size_t\)", _code(_read("adjoint.hip")))


def test_each_rule_stands_once():
    kernels, adjoint, half, ragged, vr = (_read(n) for n in ("kernels.hip", "adjoint.hip", "half_rules.h", "ragged_rules.h", "vr_ragged_rules.h"))
    # the table the two-stage form owns: asked where the exact ragged launch steps aside and where the table branch hands it over
    assert "job_two_stage_table(" in _function(kernels, "static const char *launch_ragged_job(")
    assert "job_two_stage_table(" in _function(kernels, "static const char *launch_job_table(")
    assert _code(kernels).count("job_two_stage_table(") == 2 and "no_two_stage" not in _code(adjoint)
    # the device copy of a clip table is made in one function
    both = kernels + adjoint
    uploads = [m.start() for m in re.finditer(r"hipMemcpyAsync\([^;]*clip_table\b", both)]
    assert len(uploads) == 1 and uploads[0] < len(kernels)
    made = _function(kernels, "const char *clip_table_device(")
    assert "hipMallocAsync(" in made and "clip_table," in made and kernels.index(made) <= uploads[0] < kernels.index(made) + len(made)
    assert "hipMallocAsync" not in _function(adjoint, "const char *launch_adjoint_ragged(") and "clip_table_device(" in adjoint
    # one element switch
    assert kernels.count("case HIPSOXR_I16:") == 1 and "case HIPSOXR_I16:" in _function(kernels, "static const char *with_elem(")
    # the clip-row check: three callers, one statement
    assert "job_row_check(" in kernels and "job_row_check(" in adjoint and "job_row_bounds(" in vr
    for text in (kernels, adjoint, vr):
        assert not re.search(r"r(ow)?\[0\] < 0", _code(text))
    # thresholds and limits refer to the header's
    assert re.search(r"kHalfAutoFftMin = kJobAutoFftMin;", half) and not re.search(r"kHalfAutoFftMin\s*=\s*[(\d]", half)
    assert "kHalfMaxCols = kJobMaxCols;" in half and "kMaxGridY = kJobMaxCols;" in ragged and "kMaxGridY / n_channels" in ragged
    assert "65535" not in _code(half) and "65535" not in _code(ragged)
    # the text of a missing device
    assert len(re.findall(r'"no HIP device available', kernels + adjoint + _read("engine.cpp") + _read("device.h"))) == 1


def test_no_dispatch_function_is_long():
    """launch_job is a sequence of calls: nothing of the dispatch layer is longer than about 35 lines."""
    src = _read("kernels.hip")
    layer = src[src.index("static const char *job_entry_refusal("):]
    bodies = re.findall(r"\n(?:static )?(?:const char \*|bool )(\w+)\([^;{]*\)\n\{\n(.*?)\n\}\n", layer, re.S)
    assert {"launch_job", "launch_job_table", "launch_job_engines", "launch_job_folded"} <= {n for n, _ in bodies}
    for name, body in bodies:
        assert body.count("\n") + 3 <= 36, (name, body.count("\n") + 3)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_slow_statements(build, tmp_path):
    exe = str(tmp_path / ("job_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "c", "job_rules_check.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    print(ran.stdout[-3000:])
    assert ran.returncode == 0, ran.stdout[-3000:] + ran.stderr[-3000:]
    assert re.search(r"\b[1-9]\d* checks, 0 failed", ran.stdout)
