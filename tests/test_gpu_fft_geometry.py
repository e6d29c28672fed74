"""Block sizes of one-round jobs on the frequency-domain engine (csrc/fft.hip, kOneRoundCost): 48k <-> 44.1k float32
unit-stride columns on blocks of 14 and 20 periods, beside the 8 / 16 / 32 that every element type has.

Each new block size is forced through the debug-switch build (HIPSOXR_DEBUG_FFT_K=14 / 20: every eligible job, whatever
its size), and the product library runs the same probe under its own rule.  Both directions: lengths that end just before,
on and just behind the kept run of one and of two block pairs, and on the first 16-byte granule of the next run; a 60 s
clip; two planar columns; a ragged batch through the clip table — against the oracle's float64 direct form on the
oracle's own bank at the engine's bar (<= 1e-6 relative RMS), and the same job twice gives the same bytes.

What must NOT move: the 128 x 10 s batch launches the kernel it launched before the rule existed (product result ==
result with the rule off, HIPSOXR_DEBUG_FFT_K=-1, bit for bit), and a float64 job and an int16 FFT_PCM job give the
same bytes whatever k is forced for float32 jobs — the new block sizes exist for float32 columns only."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBG_LIB = os.path.join(os.path.dirname(HERE), "python-soxr_amd", "_variants", "dbg", "libhipsoxr.so")
BAR = 1e-6


def _probe(env_extra, debug_build):
    env = {k: v for k, v in os.environ.items() if not k.startswith("HIPSOXR_")}
    env.update(env_extra)
    if debug_build:
        assert os.path.exists(DBG_LIB), "build.sh makes the debug-switch build beside the product"
        env["HIPSOXR_LIBRARY"] = DBG_LIB
    r = subprocess.run([sys.executable, os.path.join(HERE, "_geometry_probe.py")], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("GEOMETRY_PROBE ")][-1]
    return json.loads(line[len("GEOMETRY_PROBE "):])


@pytest.fixture(scope="module")
def runs():
    return {"rule": _probe({}, False), "off": _probe({"HIPSOXR_DEBUG_FFT_K": "-1"}, True),
            "k14": _probe({"HIPSOXR_DEBUG_FFT_K": "14"}, True), "k20": _probe({"HIPSOXR_DEBUG_FFT_K": "20"}, True)}


@pytest.mark.parametrize("which", ["rule", "off", "k14", "k20"])
def test_within_the_bar_of_the_oracle_and_deterministic(runs, which):
    got = runs[which]
    n = 0
    for k, v in got.items():
        if k.endswith("_deterministic"):
            assert v is True, (which, k)
        elif not k.endswith("_sha"):
            print(which, k, v)
            assert v <= BAR, (which, k, v)
            n += 1
    assert n == 2 * (16 + 3)  # both directions: 16 lengths, the 60 s clip, two planar columns, the ragged batch


def test_the_switch_switches(runs):
    """Three block sizes, three roundings: the 60 s clip's bytes differ between k = 14, k = 20 and the rule off (k = 16)."""
    for d in ("down", "up"):
        assert len({runs[w][d + "_clip60_sha"] for w in ("off", "k14", "k20")}) == 3, d


def test_large_batch_launches_what_it_launched(runs):
    """128 x 10 s: far above one round — the product's choice is the one made with the rule off, bit for bit."""
    for d in ("down", "up"):
        assert runs["rule"][d + "_batch128_sha"] == runs["off"][d + "_batch128_sha"], d


def test_float64_and_pcm_paths_did_not_move(runs):
    """float64 and int16 FFT_PCM jobs: the same bytes with the new block sizes forced, off, and under the rule."""
    for d in ("down", "up"):
        for key in (d + "_f64_sha", d + "_i16_pcm_sha"):
            assert len({runs[w][key] for w in ("rule", "off", "k14", "k20")}) == 1, key
