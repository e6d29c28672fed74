"""The one-round float32 kernels of the frequency-domain engine (csrc/fft.hip, HIPSOXR_PART5_SPECS: 2240 x 2058 and
3200 x 2940 points, both directions) can read twiddle factors from per-pass tables laid out [t][k] (as built: the third
pass of both transforms of 2240 x 2058; FFT_ONE_ROUND_TABS and pair_tabs choose) instead of forming powers of table entries.  A wrong entry or a
wrong place of a pass in the table is a wrong factor on one butterfly input of one residue class: a spur, far above the
bars below.

Both block sizes are forced through the debug-switch build (HIPSOXR_DEBUG_FFT_K = 14 and 20, one child process each,
tests/_one_round_probe.py); the launch log must name the row of the schedule table that holds them (small == 3).  Jobs:
both directions, float32 unit-stride columns; output lengths of one block pair's kept run, one more, and three pairs plus
a seeded remainder (seven blocks: an odd count); mono and a (3, n, 1) planar batch; white noise and a sum of ten tones,
one in each tenth of the pass band.  Against the oracle's float64 direct form on the oracle's own bank at the bars of
tests/test_gpu_fft.py: 1e-6 relative RMS, 4e-5 x RMS pointwise, 4e-6 x RMS per 2048-sample stretch.  The same job twice
gives the same bytes, and the 8 guard elements either side of every column stay as they were.

Accuracy: on a seeded 60 s clip at k = 14 the relative RMS error against the exact engine must not exceed the parent's
(the kernel that formed its twiddles in registers) on the same input: PARENT_CLIP60_REL, measured with the parent's
library beside this one in one visit (profiles/NOTES_one_round_chain.md)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
GUARD, POISON = 8, 12345.0
DIRS = {"down": (48000, 44100, 147, 160), "up": (44100, 48000, 160, 147)}
KS = (14, 20)
PARENT_CLIP60_REL = 2.155757320e-07  # the parent's library on this input (two runs, the same figure)


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def _signal(kind, n, fi, fo, rng):
    if kind == "noise":
        return (rng.standard_normal(n) * 0.25).astype(np.float32)
    band = 0.45 * min(fi, fo)  # the pass band of the VHQ recipe ends above 0.45 of the lower rate
    t = np.arange(n, dtype=np.float64) / fi
    x = np.zeros(n)
    for i in range(10):
        f = (i + rng.uniform(0.1, 0.9)) / 10 * band
        x += 0.08 * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    return x.astype(np.float32)


def _in_len_for(out_len, n_out, guess):
    n = guess
    while out_len(n) < n_out:
        n += 1
    while out_len(n) > n_out:
        n -= 1
    assert out_len(n) == n_out
    return n


@pytest.fixture(scope="module")
def jobs():
    """name -> (input, reference): computed once, shared by both block sizes.  name = dir_k<k>_<length>_<layout>_<input>."""
    from oracle import oracle as o
    from soxr_amd import device as dev
    rng = np.random.default_rng(2240)
    out = {}
    for d, (fi, fo, L, M) in DIRS.items():
        out_len = dev.Plan(fi, fo, "VHQ").out_len
        for k in KS:
            run = 2 * (k - 2) * L  # a block of k periods keeps k - 2 of them; a pair of blocks twice that
            for tag, n_out in (("run", run), ("run1", run + 1), ("odd", 3 * run + int(rng.integers(1, run // 2)))):
                n = _in_len_for(out_len, n_out, n_out * M // L)
                for kind in ("noise", "tones"):
                    x = np.stack([_signal(kind, n, fi, fo, rng) for _ in range(3)])
                    ref = np.stack([o.resample(x[c], fi, fo, "VHQ", mode="ref") for c in range(3)])
                    assert ref.shape[1] == n_out
                    out[f"{d}_k{k}_{tag}_mono_{kind}"] = (x[0], ref[:1])
                    out[f"{d}_k{k}_{tag}_batch_{kind}"] = (x, ref)
    return out


@pytest.fixture(scope="module")
def results(jobs, tmp_path_factory):
    """k -> the probe's results for the jobs of that block size (one child process per setting)."""
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    tmp = tmp_path_factory.mktemp("one_round_chain")
    got = {}
    for k in KS:
        mine = {"x_" + name: x for name, (x, _) in jobs.items() if f"_k{k}_" in name}
        if k == 14:
            mine["clip60"] = (np.random.default_rng(60).standard_normal(48000 * 60) * 0.25).astype(np.float32)
        np.savez(tmp / f"jobs{k}.npz", **mine)
        env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
        env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_FFT_K": str(k), "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / f"launch{k}.log")})
        r = subprocess.run([sys.executable, os.path.join(HERE, "_one_round_probe.py"), str(tmp / f"jobs{k}.npz"), str(tmp / f"results{k}.npz")],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got[k] = dict(np.load(tmp / f"results{k}.npz"))
    return got


def _names():
    return [f"{d}_k{k}_{tag}_{layout}_{kind}" for d in DIRS for k in KS for tag in ("run", "run1", "odd") for layout in ("mono", "batch")
            for kind in ("noise", "tones")]


@pytest.mark.parametrize("name", _names())
def test_against_the_oracle_guards_and_determinism(jobs, results, name):
    k = int(name.split("_")[1][1:])
    d = name.split("_")[0]
    _, ref = jobs[name]
    got = results[k]
    buf, log = got["y_" + name], str(got["log_" + name])
    L, M = DIRS[d][2], DIRS[d][3]
    # the launch: one paired-block launch on the one-round row of the schedule table
    assert log.count("\n") == 0 and "form=pair2 " in log and f" L={L} M={M} k={k} small=3 " in log and " kind=f32 " in log, log
    assert buf.shape == (ref.shape[0], ref.shape[1] + 2 * GUARD)
    assert np.all(buf[:, :GUARD] == POISON) and np.all(buf[:, -GUARD:] == POISON), "guard elements were written"
    assert bool(got["same_" + name]), "two runs of the same job differ"
    for c in range(ref.shape[0]):
        y, r = buf[c, GUARD:-GUARD].astype(np.float64), ref[c]
        err = y - r
        rel, worst = _rms(err) / _rms(r), np.abs(err).max() / _rms(r)
        seg = np.sqrt(np.mean(err[: len(err) // 2048 * 2048].reshape(-1, 2048) ** 2, axis=1)).max() / _rms(r)
        print(name, "column", c, "rel RMS %.3g  worst point %.3g x RMS  worst stretch %.3g x RMS" % (rel, worst, seg))
        assert rel <= 1e-6
        assert worst <= 4e-5
        assert seg <= 4e-6


def test_clip60_accuracy_not_worse_than_the_parent(results):
    rel = float(results[14]["clip60_rel"])
    print("60 s clip, k = 14, relative RMS against the exact engine: %.4g (parent %.4g)" % (rel, PARENT_CLIP60_REL))
    assert rel <= PARENT_CLIP60_REL
