"""GPU: randomised differential test of the gradient family (tests/fuzz/fuzz_adjoint.py: the six adjoint selectors, both C
entries, the autograd pairs) against the float64 oracle — random rate pairs, recipes, types, layouts, sizes and cotangent
lengths that no hand-written case list crosses.  What a family compares with, and the bounds (all of them the fixed tests'),
are in that file's header; tests/test_adjoint_fuzz_draw.py enumerates on the CPU what these runs do.

One child process per (family, seed) under a time limit; the first seed of a family runs on the debug-switch build with a
launch log and no switch set, the second on the product build.  After a failed child nothing further is started on the GPU
from this file.  The last test reads the launch logs of the debug-build children: every launch form of the family must have
been reached by the draw (the field names are those tests/test_gpu_adjoint_forms.py and tests/test_gpu_adjoint_two_stage.py
read) — where a form is missing, the draw is adjusted, not the assertion.

CASES per child: the time is the CPU oracle's (scatter and unit-impulse columns), measured per child in
profiles/NOTES_adjoint_fuzz.md."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DBG_LIB = os.path.join(ROOT, "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
SCRIPT = os.path.join(HERE, "fuzz", "fuzz_adjoint.py")
FAMILIES = ("exact", "interp", "fast", "ragged")
SEEDS = {"exact": (101, 102), "interp": (201, 202), "fast": (301, 302), "ragged": (401, 402)}  # (debug-switch build, product build)
CASES = {"exact": 24, "interp": 16, "fast": 32, "ragged": 16}  # (fast: 8 cases of KERNEL_ADJOINT_TWO_STAGE, so the refusal cap admits one)
TIMEOUT = 300

_stopped = []  # a failed child: nothing further is started on the GPU from this file
_done = {}     # (family, seed) -> (stdout, launch log text or None)


@pytest.fixture(autouse=True)
def _nothing_after_a_failure():
    if _stopped:
        pytest.fail("an earlier GPU step of this file failed (%s): no further GPU work from it" % _stopped[0])


def _child(family, seed, tmp_path_factory):
    if (family, seed) in _done:
        return _done[(family, seed)]
    debug = seed == SEEDS[family][0]
    env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
    log = None
    if debug:
        assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
        log = str(tmp_path_factory.mktemp("adjoint_fuzz_%s" % family) / "launch.log")
        env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": log})
    try:
        p = subprocess.run([sys.executable, SCRIPT, family, str(CASES[family]), str(seed)], env=env, capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _stopped.append("%s seed %d: time limit" % (family, seed))
        raise
    print(p.stdout[-6000:])
    if p.returncode != 0:
        _stopped.append("%s seed %d: exit status %d" % (family, seed, p.returncode))
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-3000:]
    assert "0 failures in %d cases" % CASES[family] in p.stdout
    text = None
    if debug:
        with open(log) as f:
            text = f.read()
    _done[(family, seed)] = (p.stdout, text)
    return _done[(family, seed)]


@pytest.mark.gpu
@pytest.mark.parametrize("family,seed", [(f, s) for f in FAMILIES for s in SEEDS[f]])
def test_random_adjoint_jobs_against_the_oracle(family, seed, tmp_path_factory):
    _child(family, seed, tmp_path_factory)


def _fields(line):
    return dict(tok.split("=", 1) for tok in line.split() if "=" in tok)


@pytest.mark.gpu
def test_the_draw_reached_every_launch_form(tmp_path_factory):
    lines = []
    for family in FAMILIES:
        lines += [_fields(ln) for ln in _child(family, SEEDS[family][0], tmp_path_factory)[1].splitlines()]
    census = {}

    def seen(name):
        census[name] = census.get(name, 0) + 1

    for f in lines:
        rag = " ragged" if "ragged" in f else ""
        k = f.get("kernel")
        if k == "adj_gather":
            seen("adj_gather" + rag)
        elif k == "adj_tile":
            seen("adj_tile" + rag)
            seen("adj_tile lanes=%s" % f["lanes"] + rag)
            cg = int(f["cg"])
            if cg > 1:
                seen("adj_tile cg>1 by %s" % ("shift" if cg & (cg - 1) == 0 else "division") + rag)
            if int(f["grid"].split("x")[2]) > 1:
                seen("adj_tile gz>1" + rag)
        elif k == "adj_interp":
            seen("adj_interp" + rag)
        elif k == "poly_adj":
            seen("poly_adj" + rag)
        elif "form" in f and f["form"] != "none":
            # No forward of these children runs on the frequency-domain engine (the draw's forward selector is KERNEL_EXACT), so
            # every such line is an adjoint's: the two-stage form's FFT stage runs a 2:1 / 1:2 plan, beside its poly_adj line;
            # any other ratio is KERNEL_ADJOINT_FFT's transposed plan (such a job at 2:1 is counted with the stage: no harm).
            stage = (f["L"], f["M"]) in (("2", "1"), ("1", "2"))
            seen(("fft stage" if stage else "adjoint_fft") + rag)
    print("adjoint fuzz census (launches of the debug-build children):")
    for name in sorted(census):
        print("  %-40s %d" % (name, census[name]))
    need = ["adj_gather", "adj_tile lanes=64", "adj_tile lanes=32", "adj_tile lanes=16", "adj_tile cg>1 by shift", "adj_tile cg>1 by division",
            "adj_tile gz>1", "adj_interp", "poly_adj", "fft stage", "adjoint_fft"]
    need += [n + " ragged" for n in need]  # ... and the RAGGED form of each of those
    missing = [n for n in need if n not in census]
    assert not missing, "launch forms the draw did not reach (adjust the draw, not this list): %s" % missing
