"""The oracle itself at stream positions up to 2^50 (no GPU): tests/test_gpu_window_positions.py leans on
oracle.resample_channel(..., k0=, in_abs0=) and oracle.quantize(..., k0=) as the reference of window jobs half a day and more
into a stream's life, so the reference is pinned there first.

  * The period-shift identity.  Output k0 = q L + r of a signal placed at in_abs0 reads the inputs, and multiplies by the
    coefficients, of output r of the same signal placed at in_abs0 - q M: the two runs must agree bit for bit, in the
    canonical-order ports (port_f32, port_f64) and in the long-double reference (ref), on exact-bank and interpolated-phase
    plans, at every position class and input placement the GPU test uses (tests/_window_probe.py: the outputs straddle 2^31 /
    2^32, the inputs straddle 2^32, k0 just above 2^40, 2^47, 2^50 — on L = 4800037 the product k0 M is 2^62.07 at the
    first of these and beyond 2^63 at the others).
    The moved run sits at a few thousand frames, where the rest of the suite pins the oracle against the reference library's
    known answers; a locate that wrapped or lost low bits at the large position would break the identity.
  * The zero extension: a window that starts late or ends early gives the result of the same window padded with explicit zeros.
  * quantize's dither key is the absolute output index in 64 bits: held against a statement of the hash in Python's integers
    either side of and across 2^31, 2^32, 2^40 and 2^50; a launch that crosses 2^32 equals its two halves run alone; the
    key at k and at k - 2^32 differ."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _window_probe as wp  # noqa: E402

PLANS = [(48000, 44100, "VHQ"), (44100, 16000, "VHQ"), (48000, 44101.5, "HQ"), (44100, 48000.37, "HQ")]
GEOMETRY = {PLANS[0]: (147, 160, 0), PLANS[1]: (160, 441, 0), PLANS[2]: (29401, 32000, 32), PLANS[3]: (4800037, 4410000, 32)}  # L, M, phase intervals
N_OUT = 700
MODES = {"port_f32": np.float32, "port_f64": np.float64, "ref": np.float64}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", PLANS, ids=lambda c: "%g-%g-%s" % c)
def test_period_shift_identity_and_zero_extension(oracle, case, mode):
    pl = oracle.plan(*case)
    assert (pl.L, pl.M, pl.phases) == GEOMETRY[case]
    for ci, cls in enumerate(wp.POSITIONS):
        k0, q = wp.position(pl.L, pl.M, pl.T, N_OUT, cls)
        assert wp.class_holds(pl.L, pl.M, pl.T, k0, N_OUT, cls) and k0 % pl.L != 0 and q > 0, (cls, k0)
        if case == PLANS[3] and ci >= 3:  # (d): 2^62.07, the last position a 64-bit product holds; (e), (f): beyond it
            assert k0 * pl.M > 2 ** (62 if ci == 3 else 63)
        n0, total = wp.first_tap(pl.L, pl.M, pl.T, k0), wp.span(pl.L, pl.M, pl.T, k0, N_OUT) + 5
        sig = np.random.default_rng(100 * PLANS.index(case) + ci).standard_normal(total).astype(MODES[mode])
        whole = oracle.resample_channel(pl, sig, mode, k0=k0, n_out=N_OUT, in_abs0=n0 - 5)
        assert np.isfinite(whole).all() and 0.1 < np.sqrt(np.mean(np.square(whole.astype(np.float64)))) < 10, (cls, "the window holds the signal")
        for how in wp.PLACEMENTS:
            in_abs0, n_in, lead = wp.placement(pl.L, pl.M, pl.T, k0, N_OUT, how)
            x = sig[lead:lead + n_in]
            here = oracle.resample_channel(pl, x, mode, k0=k0, n_out=N_OUT, in_abs0=in_abs0)
            moved = oracle.resample_channel(pl, x, mode, k0=k0 - q * pl.L, n_out=N_OUT, in_abs0=in_abs0 - q * pl.M)
            assert here.tobytes() == moved.tobytes(), (cls, how, "the result depends on the position, not on the phase")
            # explicit zeros where the window has none: the same numbers
            padded = sig.copy()
            padded[:lead] = 0
            padded[lead + n_in:] = 0
            assert here.tobytes() == oracle.resample_channel(pl, padded, mode, k0=k0, n_out=N_OUT, in_abs0=n0 - 5).tobytes(), (cls, how)
            if how in ("exact", "history5"):  # frames no output reads change nothing
                assert here.tobytes() == whole.tobytes(), (cls, how)
        # one output further than the window reaches, in float64: the zeros are read (the outermost taps are ~1e-9 of the centre's)
        if mode != "port_f32":
            late = oracle.resample_channel(pl, sig[5 + 40:], mode, k0=k0, n_out=N_OUT, in_abs0=n0 + 40)
            assert late[0] != whole[0] and np.array_equal(late[N_OUT // 2:], whole[N_OUT // 2:]), cls


M64 = 2 ** 64 - 1


def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _dither(seed, channel, k):
    """the TPDF dither of output k (include/hipsoxr.h: a counter-based hash of (seed, channel, absolute output index)), in Python's integers"""
    z = _mix64((k * 0x9E3779B97F4A7C15 + ((channel << 32) | seed)) & M64)
    return ((z & 0xFFFFFF) - ((z >> 24) & 0xFFFFFF)) / 16777216.0


@pytest.mark.parametrize("power", [31, 32, 40, 50])
def test_quantize_key_is_the_absolute_index_in_64_bits(oracle, power):
    seed, ch, n = 0x5EED1234, 1, 96
    k0 = 2 ** power - n // 2
    v = (np.random.default_rng(power).standard_normal(n) * 3).astype(np.float32)  # a few LSB: the dither decides most samples
    got, clips = oracle.quantize(v, np.int16, channel=ch, k0=k0, dither=True, seed=seed)
    d = np.array([_dither(seed, ch, k0 + i) for i in range(n)])
    assert [oracle.lib().oracle_dither(seed, ch, k0 + i) for i in range(n)] == list(d)
    want = np.rint(v + d.astype(np.float32)).astype(np.int16)  # (float32 sum, round half to even: what the output stage does)
    assert clips == 0 and np.array_equal(got, want)
    # the launch that crosses the power of two is its two halves
    h = n // 2
    a, _ = oracle.quantize(v[:h], np.int16, channel=ch, k0=k0, dither=True, seed=seed)
    b, _ = oracle.quantize(v[h:], np.int16, channel=ch, k0=2 ** power, dither=True, seed=seed)
    assert np.array_equal(got, np.concatenate([a, b]))
    # the other side of 2^32 has other dither, and so has the index cut to 32 bits
    for other in (k0 - 2 ** 32, k0 + 2 ** 32, (k0 + h) % 2 ** 32 - h):
        if other >= 0 and other != k0:
            assert not np.array_equal(got, oracle.quantize(v, np.int16, channel=ch, k0=other, dither=True, seed=seed)[0]), other
    # no dither: no key
    assert np.array_equal(oracle.quantize(v, np.int16, k0=k0, dither=False)[0], oracle.quantize(v, np.int16, k0=0, dither=False)[0])
