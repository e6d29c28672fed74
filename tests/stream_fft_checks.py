"""Shared checks for device streams on the frequency-domain engine (TensorStream(engine="fft")): used by
tests/test_gpu_stream_fft.py and tests/fuzz/fuzz_stream_fft.py.

Bars are the engine's own (tests/test_gpu_fft.py, tests/test_gpu_fft_pcm.py): relative RMS against the oracle's float64
direct form <= 1e-6 (float32), 2e-9 (float64 VHQ) / 1e-6 (float64 HQ: its 128 dB stop band is what the method
neglects).  Errors are normalised by the RMS of the WHOLE reference, all channels together — the engine pairs two
channels (or two blocks) in one complex transform, so its rounding is relative to the pair, not to one column — and the
same bar is held on every window of +-taps outputs around a chunk boundary and on the head and tail of the stream: a
wrong lead-in or a misplaced first block is a local error that a global RMS hides."""
import numpy as np

# rate pairs of the paired-kernel schedule table (csrc/fft.hip fft_pairs), as L/M classes
TABLE_RATES = [(48000, 44100), (44100, 48000), (44100, 16000), (16000, 44100), (48000, 16000), (16000, 48000),
               (96000, 48000), (48000, 96000), (48000, 32000), (32000, 48000), (44100, 32000), (32000, 44100),
               (88200, 48000), (96000, 44100), (44100, 8000), (192000, 44100), (22050, 32000), (44100, 12000),
               (24000, 32000), (48000, 8000), (48000, 12000)]
LEVELS = np.array([1.0, 0.5, 0.8, 0.3, 0.9, 0.6, 0.4, 0.7])  # unequal channel levels


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a ** 2))) if a.size else 0.0


def tolerance(dtype, quality):
    if np.dtype(dtype) == np.float64 and quality == "VHQ":
        return 2e-9
    return 1e-6


def signal(rng, frames, ch, dtype, full_scale=False):
    """White noise, unequal channel levels; integers in LSB units (full_scale: +-32767 runs, the filter's overshoot clips)."""
    dtype = np.dtype(dtype)
    shape = (frames, ch) if ch > 1 else (frames,)
    lev = LEVELS[:ch] if ch > 1 else 1.0
    if dtype == np.int16:
        if full_scale:
            n = int(np.prod(shape))
            runs = rng.integers(1, 40, size=max(n, 1))
            sign = np.repeat(np.where(rng.random(max(n, 1)) < 0.5, -32767, 32767), runs)[:n]
            return sign.reshape(shape).astype(np.int16)
        return np.clip(np.rint(rng.standard_normal(shape) * 5000 * lev), -32768, 32767).astype(np.int16)
    if dtype == np.int32:
        return np.clip(np.rint(rng.standard_normal(shape) * 2.0 ** 27 * lev), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int32)
    return (rng.standard_normal(shape) * 0.25 * lev).astype(np.float32).astype(dtype)  # (float32-representable: one reference serves both widths)


def random_plan(r, total, max_chunk=200000):
    """Seeded random chunk sizes from 1 to max_chunk frames that add up to `total` (r: random.Random)."""
    sizes, left = [], total
    while left > 0:
        n = min(left, r.choice([1, r.randint(2, 500), r.randint(500, 6000), r.randint(6000, 50000), r.randint(50000, max_chunk)]))
        sizes.append(n)
        left -= n
    return sizes


def torch_dtype(dtype):
    import torch
    return torch.from_numpy(np.zeros(1, dtype)).dtype


def feed(ts, x, sizes, twin=None):
    """Feed x in chunks of `sizes` (the last one with last=True).  Returns (outputs per call as numpy, delays after each
    call).  twin: a second stream fed the same chunks; its per-call counts and delays must be the same."""
    import torch
    xt = torch.from_numpy(x).cuda()
    outs, pos = [], 0
    for i, n in enumerate(sizes):
        last = i == len(sizes) - 1
        chunk = xt[pos:pos + n]
        pos += n
        y = ts.resample_chunk(chunk, last=last)
        if twin is not None:
            w = twin.resample_chunk(chunk, last=last)
            assert y.shape == w.shape, f"call {i} ({n} frames, last={last}): {tuple(y.shape)} frames, the default stream returns {tuple(w.shape)}"
            if not last:
                assert ts.delay() == twin.delay(), (i, ts.delay(), twin.delay())
        outs.append(y.cpu().numpy())
    assert pos == x.shape[0]
    return outs


def check_values(outs, ref, taps, tol, what=""):
    """Concatenated outputs against the float64 reference: the bar globally, and on a window of +-taps outputs around every
    chunk boundary, on the head and on the tail — each normalised by the RMS of the whole reference.  Prints every figure."""
    y = np.concatenate(outs).astype(np.float64)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    scale = rms(ref)
    err = y - ref
    worst = rms(err) / scale
    print(f"{what}: global {worst:.3e} (bar {tol:.1e})", end="")
    assert worst <= tol, (what, "global", worst)
    bounds = np.cumsum([len(o) for o in outs])[:-1]
    wins = [(0, min(taps, len(y))), (max(len(y) - taps, 0), len(y))] + [(max(b - taps, 0), min(b + taps, len(y))) for b in bounds]
    seam = 0.0
    for a, b in wins:
        if b > a:
            e = rms(err[a:b]) / scale
            seam = max(seam, e)
            assert e <= tol, (what, "window", a, b, e)
    print(f", worst of {len(wins)} seam windows {seam:.3e}")
    return worst, seam


def host_stage(oracle, yf, dtype, dither, seed):
    """Float stream result [frames(, channels)] -> (integers, clip count) through oracle.quantize per column, output index from 0."""
    y2 = yf[:, None] if yf.ndim == 1 else yf
    out = np.empty(y2.shape, dtype)
    clips = 0
    for c in range(y2.shape[1]):
        q, n = oracle.quantize(np.ascontiguousarray(y2[:, c]), dtype, channel=c, k0=0, dither=dither, seed=seed)
        out[:, c] = q
        clips += n
    return (out[:, 0] if yf.ndim == 1 else out), clips


def check_integer_identity(oracle, dev, in_rate, out_rate, quality, x, sizes, dither, seed, what=""):
    """Integer engine="fft" stream == float engine="fft" stream of the same arithmetic width on the same values and chunks,
    then oracle.quantize — sample for sample, clip count included (dither keyed by the ABSOLUTE output index); int16 within
    1 LSB of the default stream.  Returns the clip count."""
    import torch
    ch = 1 if x.ndim == 1 else x.shape[1]
    ftype = np.float32 if x.dtype == np.int16 else np.float64
    ti = dev.TensorStream(in_rate, out_rate, ch, dtype=torch_dtype(x.dtype), quality=quality, dither=dither, dither_seed=seed, engine="fft")
    tf = dev.TensorStream(in_rate, out_rate, ch, dtype=torch_dtype(ftype), quality=quality, engine="fft")
    yi = np.concatenate(feed(ti, x, sizes))
    yf = np.concatenate(feed(tf, x.astype(ftype), sizes))
    want, clips = host_stage(oracle, yf, x.dtype, dither, seed)
    ndiff = int(np.count_nonzero(yi != want))
    got_clips = ti.num_clips()
    print(f"{what}: {ndiff} of {yi.size} differ from float stream + quantize; clips device {got_clips} host {clips}")
    assert yi.shape == want.shape and ndiff == 0, (what, ndiff)
    assert got_clips == clips, (what, got_clips, clips)
    if x.dtype == np.int16:
        te = dev.TensorStream(in_rate, out_rate, ch, dtype=torch.int16, quality=quality, dither=dither, dither_seed=seed)
        ye = np.concatenate(feed(te, x, sizes))
        d = int(np.abs(yi.astype(np.int32) - ye.astype(np.int32)).max()) if yi.size else 0
        print(f"{what}: max |fft - exact| = {d} LSB")
        assert d <= 1, (what, d)
    return clips
