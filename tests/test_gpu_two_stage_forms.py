"""GPU: every launch form of the two-stage form's polyphase stage (csrc/twostage.hip, launch_poly) against the exact engine.

launch_poly decides (csrc/poly_rules.h): k_poly with one channel per pass, or k_poly2 on interleaved channel pairs (il=1) or on
the two segments of a split column (split=1); the window in registers for MQ 0 and 1; channel groups lg_cg; the run length R,
the lane order, the LDS bytes and the grid.  The debug-switch build writes one line per polyphase launch
(HIPSOXR_DEBUG_LAUNCH_LOG), so a case here names the form its launch must show and the test reads it from the log — the rules
are not restated.  All jobs run in ONE child process (tests/_two_stage_forms_probe.py) into guarded, NaN-filled buffers;
everything is compared here.

Per case: the launch form; 8 guard elements either side of every column untouched and every payload element written; the job
against the same job under KERNEL_EXACT at the bars of tests/test_gpu_two_stage.py — relative RMS <= 1e-6 (float32) /
2e-9 (float64), the first and last 64 outputs within 8 * tol * 0.25 absolutely (white noise of RMS 0.25).  Each case has the
smallest length the rules give its form: 8192 frames on the shorter side, or — a split column — the first length poly_form
splits (more than ~1.7 periods of Ls outputs in the polyphase launch; one frame fewer does not split).  A case is resized,
never its assertion changed, if a later launch rule moves it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
GUARD, POISON = 8, 12345.0
F32, F64 = "f32", "f64"
DTYPE = {F32: np.float32, F64: np.float64}
TOL = {F32: 1e-6, F64: 2e-9}

DOWN, UP = (48000, 44101, "VHQ"), (44101, 48000, "VHQ")          # Ms / Ls = 24000 / 44101 (MQ 0), 44101 / 24000 (MQ 1): 16 and 28 taps
DOWN_HQ, UP_HQ = (48000, 44101, "HQ"), (44101, 48000, "HQ")      # 12 and 20 taps
STEEP = (96000, 26001, "VHQ")                                    # 48 taps: beyond k_poly2's instances; the float64 table leaves LDS
THIRD, THIRD_UP = (48000, 32001, "VHQ"), (32001, 48000, "VHQ")   # Ls = 10667 (down), 8000 (up): short periods, columns of 8192+ frames split
# (at HQ these two ratios have exact banks of 10667 / 16000 phases: not interpolated plans, no two-stage form)

# name -> (plan, frames, clips, channels, layout, type, {log field: value} or None: no polyphase launch)
FORMS = {
    # k_poly: more than 40 taps (no k_poly2 instance); a mono column too short to split; float64 in both directions
    "long_taps_f32": (STEEP, 30245, 1, 1, "inter", F32, dict(kernel="poly", T=48, MQ=1, il=0, split=0)),
    "short_mono_f32": (THIRD, 12287, 1, 1, "inter", F32, dict(kernel="poly", T=20, MQ=0, il=0, split=0)),
    "up_f64": (UP, 8192, 1, 1, "inter", F64, dict(kernel="poly", width=8, MQ=1, il=0, split=0)),
    "down_f64": (DOWN, 8916, 1, 1, "inter", F64, dict(kernel="poly", width=8, MQ=0, il=0, split=0)),
    # k_poly2 on interleaved channel pairs: both window steps; 4 and 8 channels (2 and 4 pairs per workgroup)
    "pair_mq0": (DOWN, 8916, 1, 2, "inter", F32, dict(kernel="poly2", MQ=0, il=1, split=0, lg_cg=0, cols=1)),
    "pair_mq1": (UP, 8192, 1, 2, "inter", F32, dict(kernel="poly2", MQ=1, il=1, split=0, lg_cg=0, cols=1)),
    "pair_4ch": (DOWN_HQ, 8916, 1, 4, "inter", F32, dict(kernel="poly2", il=1, split=0, lg_cg=1, cols=1)),
    "pair_8ch": (UP_HQ, 8192, 1, 8, "inter", F32, dict(kernel="poly2", il=1, split=0, lg_cg=2, cols=1)),
    # k_poly2 on a split column: 13564 / 9067 frames are the first lengths that split (polyphase launches of 18134 = 1.7 x 10667
    # and 13600 = 1.7 x 8000 outputs); member 2 ends inside a tile
    "split_mono_down": (THIRD, 13564, 1, 1, "inter", F32, dict(kernel="poly2", MQ=0, il=0, split=1, n_out=10667, m2_n_out=7467)),
    "split_mono_up": (THIRD_UP, 9067, 1, 1, "inter", F32, dict(kernel="poly2", MQ=1, il=0, split=1, n_out=8000, m2_n_out=5600)),
    # planar stereo, three interleaved channels (no pair: an odd count), a batch of three stereo clips
    "split_planar2": (THIRD, 13564, 1, 2, "planar", F32, dict(kernel="poly2", il=0, split=1, lg_cg=0, cols=2, n_out=10667, m2_n_out=7467)),
    "split_inter3": (THIRD_UP, 9067, 1, 3, "inter", F32, dict(kernel="poly2", il=0, split=1, lg_cg=0, cols=3, n_out=8000, m2_n_out=5600)),
    "pair_3clips": (DOWN, 8916, 3, 2, "inter", F32, dict(kernel="poly2", il=1, split=0, cols=3)),
    # the float64 table of a 48-tap stage (128 x 49 records of 32 bytes) does not fit LDS: the exact engine keeps the job
    "no_fit_f64": (STEEP, 30245, 1, 1, "inter", F64, None),
}


def _parse(line):
    """one polyphase launch line -> {field: value}; grid=XxYxZ becomes gx, gy, gz"""
    f = dict(tok.split("=", 1) for tok in line.split())
    out = {k: (v if k == "kernel" else float(v) if k == "conf" else int(v)) for k, v in f.items() if k != "grid"}
    out["gx"], out["gy"], out["gz"] = (int(v) for v in f["grid"].split("x"))
    return out


@pytest.fixture(scope="module")
def jobs():
    """name -> x [clips, frames, channels]: white noise of RMS 0.25, every column its own"""
    rng = np.random.default_rng(5151)
    return {n: (rng.standard_normal((clips, frames, ch)) * 0.25).astype(DTYPE[kind]) for n, (_, frames, clips, ch, _, kind, _) in FORMS.items()}


@pytest.fixture(scope="module")
def results(jobs, tmp_path_factory):
    """The probe's results: one child process for the whole file."""
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    tmp = tmp_path_factory.mktemp("two_stage_forms")
    meta = [{"name": n, "case": list(FORMS[n][0]), "layout": FORMS[n][4]} for n in jobs]
    np.savez(tmp / "jobs.npz", meta=np.array(json.dumps(meta)), **{"x_" + n: x for n, x in jobs.items()})
    env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
    env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / "launch.log")})
    r = subprocess.run([sys.executable, os.path.join(HERE, "_two_stage_forms_probe.py"), str(tmp / "jobs.npz"), str(tmp / "results.npz")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(tmp / "results.npz")


def _rms(v):
    return float(np.sqrt(np.mean(np.square(v, dtype=np.float64))))


@pytest.mark.parametrize("name", list(FORMS))
def test_form_guards_and_parity(results, name):
    case, frames, clips, ch, layout, kind, expect = FORMS[name]
    log = str(results["log_" + name])
    poly = [ln for ln in log.splitlines() if ln.startswith("kernel=poly")]
    print(name, "launches:", log.replace("\n", " | "))
    buf, ye = results["y_" + name], results["ye_" + name]
    n_out = ye.shape[1]
    assert min(frames, n_out) >= 8192, "the two-stage form takes jobs of 8192 frames either side"
    assert ye.shape == (clips, n_out, ch) and buf.shape == (clips, n_out + 2 * GUARD, ch) and buf.dtype == ye.dtype == DTYPE[kind]
    assert np.all(buf[:, :GUARD] == POISON) and np.all(buf[:, -GUARD:] == POISON), "guard elements were written"
    y = buf[:, GUARD:-GUARD]
    assert np.isfinite(y).all(), "a payload element was not written"
    if expect is None:
        assert not poly, "a polyphase launch for a job whose table does not fit LDS"
        assert np.array_equal(y, ye), "AUTO left the exact engine without taking the two-stage form"
        return
    assert len(poly) == 1, "one polyphase launch per job: %r" % log
    f = _parse(poly[0])
    assert f["width"] == (4 if kind == F32 else 8) and f["block"] == 256
    assert {k: f[k] for k in expect} == expect, f
    # what every launch shows: the kernel family, the tile count of member 1, a grid within it, LDS within a workgroup's
    assert (f["kernel"] == "poly2") == bool(f["il"] or f["split"]) and not (f["il"] and f["split"])
    assert 1 <= f["R"] <= 12 and f["lane_mul"] % 2 == 1 and f["tiles"] == -(-f["n_out"] // (256 * f["R"]))
    assert 1 <= f["gx"] <= f["tiles"] and f["gy"] == f["cols"] == clips * ch // ((2 if f["il"] else 1) << f["lg_cg"]) and f["gz"] == 1
    assert f["lds"] <= 160 * 1024
    if f["split"]:  # member 1 is the longer one; member 2 ends inside a tile
        assert 0 < f["m2_n_out"] <= f["n_out"] and f["m2_n_out"] % (256 * f["R"]) != 0
    else:
        assert f["m2_n_out"] == f["n_out"]
    tol = TOL[kind]
    d = y.astype(np.float64) - ye
    rel = _rms(d) / _rms(ye)
    ends = max(float(np.abs(d[:, :64]).max()), float(np.abs(d[:, -64:]).max()))
    print("two-stage forms %s: relative RMS %.3g (bar %.0e), ends %.3g (bar %.3g)" % (name, rel, tol, ends, 8 * tol * 0.25))
    assert not np.array_equal(y, ye), "the exact engine's bits: the polyphase launch did not write the result"
    assert rel <= tol, rel
    assert ends <= 8 * tol * 0.25, ends
