"""The device-job dispatcher (csrc/kernels.hip launch_job, rules in csrc/job_rules.h) decides what it decided before it was
split: every job of tests/job_dispatch_cases.py — around the AUTO threshold of 2^13 outputs for every element type, as equal-
length jobs and as clip tables; the selector refusals; an interpolated-phase plan on and off the two-stage form; every kind of
invalid clip row; the clip loop; the fold with both axes wide — is answered with the refusal text, or the kernel names, number
of launches and column counts, that tests/golden/job_dispatch.json holds.  That fixture was recorded once from the debug-switch
library of the commit BEFORE the split (tests/golden/make_job_dispatch_golden.py), never from the code under test.

One probe child per environment (default, HIPSOXR_NO_FFT, HIPSOXR_NO_TWO_STAGE: the switches are read once per process), side
by side, on the debug-switch build with HIPSOXR_DEBUG_LAUNCH_LOG.  Served jobs are also checked for what they computed: on the
exact engine bit for bit against KERNEL_EXACT of the same job; in the frequency-domain / two-stage class within the bars of
tests/test_gpu_two_stage.py (float32) and tests/test_gpu_fft.py (float64 on this plan) against the same; float16 jobs by the
identity of tests/test_gpu_half.py (the float32 job of the same selector on the widened values, rounded once)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from job_dispatch_cases import CASES, ENVS, EXACT, EXACT_PLAN, FOLD, WAVE_DOT
import test_gpu_fft as fft_module  # (modules, not their test functions: a name test_* here would be collected again)
import test_gpu_two_stage as two_stage_module

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DBG_LIB = os.path.join(ROOT, "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
EXACT_KERNELS = ("gather_wave", "chain", "interp_wave", "interp_tile", "interp", "gather", "tile", "tile_mfma", "tile_mfma_p", "tile_mfma64_p")


def _marks(fn, names):
    return [m.args[1] for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == names][0]


# the bars of the 1e-6 class against the exact engine, as the modules of the two engines hold them
_rms = fft_module._rms
TOL = {"f32": dict((np.dtype(d).name, t) for d, t in _marks(two_stage_module.test_two_stage_matches_the_oracle_direct_form, "dtype,tol"))["float32"],
       "f64": [t for a, b, q, t in _marks(fft_module.test_fft_engine_float64_instance, "in_rate,out_rate,quality,tol") if (a, b, q) == EXACT_PLAN][0]}
PCM_LSB = 1  # int16 by name on the frequency-domain engine: within one step of the exact engine (tests/test_gpu_fft_pcm.py)

with open(os.path.join(HERE, "golden", "job_dispatch.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("job_dispatch")
    children = {}
    for name, extra in ENVS.items():
        env = {k: v for k, v in os.environ.items() if not k.startswith("HIPSOXR_")}
        env.update(extra)
        env["HIPSOXR_LIBRARY"] = DBG_LIB
        env["HIPSOXR_DEBUG_LAUNCH_LOG"] = str(tmp / (name + ".log"))
        cmd = [sys.executable, os.path.join(HERE, "_job_dispatch_probe.py"), name, str(tmp / (name + ".json")), str(tmp / (name + ".npz"))]
        children[name] = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    records, arrays = {}, {}
    for name, child in children.items():
        out, _ = child.communicate(timeout=600)
        assert child.returncode == 0, out[-3000:]
        with open(tmp / (name + ".json")) as f:
            records.update(json.load(f))
        with np.load(tmp / (name + ".npz")) as z:
            arrays.update({k: z[k] for k in z.files})
    return records, arrays


def test_the_fixture_covers_the_cases():
    assert sorted(GOLDEN) == sorted(c["name"] for c in CASES)
    served = [g for g in GOLDEN.values() if "lines" in g]
    assert len(served) >= 40 and sum("error" in g for g in GOLDEN.values()) >= 14
    # the decisions the cases are there for do flip in it
    kern = {n: [ln["kernel"] for ln in g.get("lines", [])] for n, g in GOLDEN.items()}
    for dt in ("f32", "f64", "f16"):
        for form in ("mono", "stereo", "table"):
            below, at = kern[f"{form}_{dt}_below"], kern[f"{form}_{dt}_at"]
            assert not [k for k in below if k.startswith("fft:")] and [k for k in at if k.startswith("fft:")], (dt, form, below, at)
    for form in ("mono", "stereo", "table"):
        assert kern[f"{form}_i16_at"] and not [k for k in kern[f"{form}_i16_at"] if k.startswith("fft:")]
    assert [k for k in kern["mono_f32_below_fft"] if k.startswith("fft:")] and not [k for k in kern["nofft_mono_f32_at"] if k.startswith("fft:")]
    assert [k for k in kern["interp_table_auto"] if k.startswith("poly")] and not [k for k in kern["interp_table_no_two_stage"] if k.startswith("poly")]
    assert [k for k in kern["interp_8192_auto"] if k.startswith("poly")] and not [k for k in kern["interp_8191_auto"] if k.startswith("poly")]
    assert "error" in GOLDEN["interp_8191_fft"] and "lines" in GOLDEN["interp_8192_fft"]
    assert len(kern["table_f16_clip_loop"]) == 2 and len(kern["table_f16_below"]) == 3 and kern["table_wave_dot_all_empty"] == []
    assert [ln["cols"] for ln in GOLDEN[FOLD]["lines"]] == [65535, 65535, 2]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_decision(probe, case):
    records, arrays = probe
    name, got, want = case["name"], probe[0][case["name"]], GOLDEN[case["name"]]
    print(name, got)
    assert got == want
    if "error" in want:
        return
    y, kernels = arrays["y_" + name], [ln["kernel"] for ln in want["lines"]]
    if int(case["kernel"]) == WAVE_DOT:  # (the reference-point kernel sums a float32 product in another order: the class bar, not bits)
        ref = arrays["ref_" + name].astype(np.float64)
        assert _rms(y - ref) <= TOL[case["dtype"]] * _rms(ref)
    elif case["dtype"] == "f16" or all(k in EXACT_KERNELS for k in kernels):
        if int(case["kernel"]) != EXACT:
            assert np.array_equal(y, arrays["ref_" + name])
    elif case["dtype"] == "i16":
        assert np.abs(y.astype(np.int32) - arrays["ref_" + name].astype(np.int32)).max() <= PCM_LSB
    else:  # the frequency-domain engine or the two-stage form took it (or a part of a table)
        ref = arrays["ref_" + name].astype(np.float64)
        assert _rms(ref) > 0 and _rms(y - ref) <= TOL[case["dtype"]] * _rms(ref), _rms(y - ref) / _rms(ref)


def test_fold_keeps_the_dither_key(probe):
    """65536 clips x 2 channels, int16 with dither: folded over clip ranges and the first range again over its channels.  Every
    column equals the same column of the job cut by hand into clip ranges that need no fold, where a channel's dither is keyed
    by its index in the job — and the two channels, fed the same samples, differ: the key is at work."""
    _, arrays = probe
    y, cut = arrays["y_" + FOLD], arrays["cut_" + FOLD]
    assert y.shape == cut.shape and y.shape[0] == 65536 and y.shape[2] == 2
    assert np.array_equal(y, cut)
    for a, b in ((65534, 65535), (65535, 65536)):  # either side of the clip boundary, both sides of the channel boundary
        assert np.array_equal(y[a:b], cut[a:b])
    assert (y[:, :, 0] != y[:, :, 1]).any()
