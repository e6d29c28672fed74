"""The one-round float32 kernels of 14 periods (csrc/fft.hip, k_fft_pair2 on 2240 x 2058 points, both directions) run
their radix-14 passes in the lane-pair form (fft_pass_pair14): two neighbouring lanes share a butterfly, each takes one
residue class of its inputs through a 7-point transform, and the 2-point stage crosses the lanes through DPP.  A wrong
residue map, a wrong twiddle base or a wrong sign moves or negates one class of outputs of every butterfly: an error of
the size of the signal, far above the bars below.

The block size is forced through the debug-switch build (HIPSOXR_DEBUG_FFT_K = 14, one child process,
tests/_one_round_probe.py); the launch log must name the one-round row of the schedule table (small == 3).  Jobs, both
directions, float32 unit-stride columns: output lengths of exactly one block pair's kept run (one workgroup: the first and
the last item of its column at once), one more (a second pair, nearly empty), and five blocks — two pairs plus a seeded
remainder: an odd block count with an interior item; mono and a (3, n, 1) planar batch of white noise, and on the
five-block length a unit impulse at each of 32 consecutive input positions inside the interior item (one planar column
each: both lane parities, every residue class).  Against the oracle's float64 direct form on the oracle's own bank at the
bars of tests/test_gpu_fft.py: 1e-6 relative RMS, 4e-5 x RMS pointwise.  The same job twice gives the same bytes, and the
8 guard elements either side of every column stay as they were."""
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
KS = (14,)  # (the kernels of 20 periods keep the plain passes)
TAGS = ("run", "run1", "five")
N_IMPULSES = 32


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


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
    """name -> (input, reference): computed once.  name = dir_k<k>_<length>_<layout>_<input>."""
    from oracle import oracle as o
    from soxr_amd import device as dev
    rng = np.random.default_rng(1414)
    out = {}
    for d, (fi, fo, L, M) in DIRS.items():
        out_len = dev.Plan(fi, fo, "VHQ").out_len
        for k in KS:
            run = 2 * (k - 2) * L  # a block of k periods keeps k - 2 of them; a pair of blocks twice that
            for tag, n_out in zip(TAGS, (run, run + 1, 2 * run + int(rng.integers(1, run // 2)))):
                n = _in_len_for(out_len, n_out, n_out * M // L)
                x = (rng.standard_normal((3, n)) * 0.25).astype(np.float32)
                ref = np.stack([o.resample(x[c], fi, fo, "VHQ", mode="ref") for c in range(3)])
                assert ref.shape[1] == n_out
                out[f"{d}_k{k}_{tag}_mono_noise"] = (x[0], ref[:1])
                out[f"{d}_k{k}_{tag}_batch_noise"] = (x, ref)
                if tag == "five":  # the middle of the signal lies in block 2 of 5: the second pair, the interior item
                    xi = np.zeros((N_IMPULSES, n), np.float32)
                    xi[np.arange(N_IMPULSES), n // 2 + np.arange(N_IMPULSES)] = 1.0
                    refi = np.stack([o.resample(xi[c], fi, fo, "VHQ", mode="ref") for c in range(N_IMPULSES)])
                    out[f"{d}_k{k}_{tag}_batch_impulses"] = (xi, refi)
    return out


@pytest.fixture(scope="module")
def results(jobs, tmp_path_factory):
    """k -> the probe's results for the jobs of that block size (one child process per setting)."""
    assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
    tmp = tmp_path_factory.mktemp("one_round_split")
    got = {}
    for k in KS:
        np.savez(tmp / f"jobs{k}.npz", **{"x_" + name: x for name, (x, _) in jobs.items() if f"_k{k}_" in name})
        env = {key: v for key, v in os.environ.items() if not key.startswith("HIPSOXR_")}
        env.update({"HIPSOXR_LIBRARY": DBG_LIB, "HIPSOXR_DEBUG_FFT_K": str(k), "HIPSOXR_DEBUG_LAUNCH_LOG": str(tmp / f"launch{k}.log")})
        r = subprocess.run([sys.executable, os.path.join(HERE, "_one_round_probe.py"), str(tmp / f"jobs{k}.npz"), str(tmp / f"results{k}.npz")],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got[k] = dict(np.load(tmp / f"results{k}.npz"))
    return got


def _names():
    names = [f"{d}_k{k}_{tag}_{layout}_noise" for d in DIRS for k in KS for tag in TAGS for layout in ("mono", "batch")]
    return names + [f"{d}_k{k}_five_batch_impulses" for d in DIRS for k in KS]


@pytest.mark.parametrize("name", _names())
def test_against_the_oracle_guards_and_determinism(jobs, results, name):
    d, k = name.split("_")[0], int(name.split("_")[1][1:])
    _, ref = jobs[name]
    got = results[k]
    buf, log = got["y_" + name], str(got["log_" + name])
    L, M = DIRS[d][2], DIRS[d][3]
    # the launch: one paired-block launch on the one-round row of the schedule table
    assert log.count("\n") == 0 and "form=pair2 " in log and f" L={L} M={M} k={k} small=3 " in log and " kind=f32 " in log, log
    assert buf.shape == (ref.shape[0], ref.shape[1] + 2 * GUARD)
    assert np.all(buf[:, :GUARD] == POISON) and np.all(buf[:, -GUARD:] == POISON), "guard elements were written"
    assert bool(got["same_" + name]), "two runs of the same job differ"
    worst_rel = worst_pt = 0.0
    for c in range(ref.shape[0]):
        y, r = buf[c, GUARD:-GUARD].astype(np.float64), ref[c]
        err = y - r
        rel, worst = _rms(err) / _rms(r), np.abs(err).max() / _rms(r)
        worst_rel, worst_pt = max(worst_rel, rel), max(worst_pt, worst)
        print(name, "column", c, "rel RMS %.3g  worst point %.3g x RMS" % (rel, worst))
        assert rel <= 1e-6
        assert worst <= 4e-5
    print(name, "worst column: rel RMS %.3g  worst point %.3g x RMS" % (worst_rel, worst_pt))
