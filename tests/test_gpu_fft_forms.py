"""The launch forms of the frequency-domain engine that tests/test_gpu_fft_table.py does not see (csrc/fft.hip,
launch_fft_impl): window jobs (the chunks of HIPSOXR_STREAM_FFT streams), a ragged batch, the wave form and its bar,
k_fft_block, "none" (declined: the caller's error, or the exact engine under AUTO), the two-stage form's inner call
(in_abs0 != 0), and one small job per instance kind and layout at 48k -> 44.1k VHQ — one to three work items per column.

tests/_fft_forms_probe.py runs them on the debug-switch build in three child processes, one after another (plain / wave /
nopair: its CHILDREN), every job into a NaN-filled buffer with guards and against the oracle at the bars of
tests/test_gpu_fft.py and tests/test_gpu_fft_pcm.py.  Every line the launch log (HIPSOXR_DEBUG_LAUNCH_LOG) holds for a case
must name the form, instance kind, ratio and window flag the case exists for (EXPECT below).

The probe also reports, per case, the whole lines as text, digests of the results and whether the one-round rule — which
reads the device's CU count — may move the case's row: what a recording of the lines on one build is compared with on
another (profiles/NOTES_fft_launch_refactor.md §4)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
# What each case must be served by, from the issue that asked for this test and from the engine's documented forms — not
# from the code under test: per launch-log line of the case (form, kind), the window flag, and the ratio where it is not
# the job's own.  "+": one or more such lines.  Integer cases run the float job of the same arithmetic width behind the
# integer one (the identity they are checked by), hence two lines.
D, U = ("147", "160"), ("160", "147")     # L, M of 48k -> 44.1k and 44.1k -> 48k
EXPECT = {
    "mono_f32": (D, "0", [("pair2", "f32")]), "ragged_f32": (D, "0", [("pair2", "f32")]),
    "il2_f32": (D, "0", [("strided2_cp", "f32")]), "il3_f32": (D, "0", [("strided2_st", "f32")]),
    "mono_f64": (D, "0", [("pair2", "f64")]), "mono_f32on64": (D, "0", [("pair2", "f32on64")]),
    "mono_i16": (D, "0", [("pair2", "i16"), ("pair2", "f32")]), "il2_i16": (D, "0", [("strided2_cp", "i16"), ("strided2_cp", "f32")]),
    "mono_i32": (D, "0", [("pair2", "i32"), ("pair2", "f64")]),
    "stream_mono_f32": (D, "1", "+", ("pair2", "f32")), "stream_il2_f32": (D, "1", "+", ("strided2_cp", "f32")),
    "block_f32": (("5", "6"), "0", [("block", "f32")]),
    "none_f64_refused": (("5", "6"), "0", [("none", "f64")]), "none_f64_auto": (("5", "6"), "0", [("none", "f64")]),
    "two_stage_down_f32": (("1", "2"), "0", "+", ("pair2", "f32")),
    "wave_barred_f32": (U, "0", [("pair2", "f32")]), "wave_f32": (U, "0", [("wave", "f32")]),
    "nopair_block_f32": (D, "0", [("block", "f32")]),
    "nopair_none_f64_refused": (D, "0", [("none", "f64")]), "nopair_none_f64_auto": (D, "0", [("none", "f64")]),
}


def _children():
    """child -> switches, read from the probe's source without importing it (it initialises the GPU on import)."""
    import ast
    with open(os.path.join(HERE, "_fft_forms_probe.py")) as f:
        for node in ast.parse(f.read()).body:
            if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "CHILDREN":
                return ast.literal_eval(node.value)
    raise AssertionError("CHILDREN not found in _fft_forms_probe.py")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    cases, cus = {}, set()
    for name, switches in _children().items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("HIPSOXR_")}
        env.update(switches)
        env["HIPSOXR_LIBRARY"] = DBG_LIB
        env["HIPSOXR_DEBUG_LAUNCH_LOG"] = str(tmp_path_factory.mktemp("forms_log") / (name + ".log"))
        r = subprocess.run([sys.executable, os.path.join(HERE, "_fft_forms_probe.py"), name], env=env, capture_output=True, text=True, timeout=600)
        started = [l for l in r.stdout.splitlines() if l.startswith("FORMS_CASE ")]
        assert r.returncode == 0, (name, "last case started: " + (started[-1] if started else "none"), r.stderr[-2000:])
        got = json.loads([l for l in r.stdout.splitlines() if l.startswith("FORMS_PROBE ")][-1][len("FORMS_PROBE "):])
        cus.add(got["cus"])
        assert not set(got["cases"]) & set(cases)
        cases.update(got["cases"])
    assert len(cus) == 1
    return cus.pop(), cases


def _fields(line):
    return dict(kv.split("=", 1) for kv in line.split())


def test_the_probe_runs_every_case(runs):
    assert set(runs[1]) == set(EXPECT)


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_values_form_and_kind(runs, name):
    """Values, guards and refusals (the probe's own checks), and every launch-log line of the case names the form, kind,
    ratio and window flag the case exists for."""
    got = runs[1][name]
    print(name, got["figs"])
    for line in got["lines"]:
        print("   ", line)
    assert not got["fails"], got["fails"]
    (L, M), window, want = EXPECT[name][0], EXPECT[name][1], EXPECT[name][2]
    # the log holds every launcher's lines.  launch_fft_impl's begin with form=; the polyphase launch of a two-stage job
    # (twostage.hip) writes one of its own, which tests/test_gpu_two_stage_forms.py reads; a job the engine declines under AUTO
    # is the exact engine's, whose tile launch (kernels.hip) writes one too, which tests/test_gpu_tile_forms.py reads
    other = [l for l in got["lines"] if not l.startswith("form=")]
    poly, tile = [l for l in other if l.startswith("kernel=poly")], [l for l in other if l.startswith("kernel=tile") and "ragged=" not in l]
    assert len(poly) == (1 if name.startswith("two_stage") else 0) and len(tile) == (1 if name.endswith("none_f64_auto") else 0) and len(other) == len(poly) + len(tile), other
    lines = [_fields(l) for l in got["lines"] if l.startswith("form=")]
    if want == "+":
        assert lines, "no launch was logged"
        want = [EXPECT[name][3]] * len(lines)
    assert [(l["form"], l["kind"]) for l in lines] == want
    for l in lines:
        assert (l["L"], l["M"], l["window"]) == (L, M, window), l
        if l["form"] == "none" and name.startswith("nopair"):
            assert (l["k"], l["small"]) == ("0", "-1"), l           # no row was chosen
