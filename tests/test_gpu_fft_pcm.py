"""HIPSOXR_KERNEL_FFT_PCM: the frequency-domain engine on int16 / int32 device jobs.

The main criterion needs no tolerance: the integer kernels are the float kernels of the same arithmetic width (float32 for
int16, float64 for int32) with the exact engine's output stage behind them, so an integer job must equal the float job on
the same values and layout pushed through `oracle.quantize` (the host restatement of that stage) — sample for sample, clip
count included.  Both jobs choose the same kernel geometry: the size rules look at the shape and the arithmetic width only
(float32 jobs of 44.1k -> 48k leave k_fft_pair2 from 8192 block pairs; every case here is far smaller).

Further: within 1 LSB of the exact engine (int16: the float engine's bar of tests/test_gpu_fft.py, max error
<= 4e-5 x RMS = 0.2 LSB at RMS 5000, so a rounded value moves by one step at most); within the float64 instance's bars of
the float64 reference plus the rounding itself (int32); refusals; AUTO untouched; the corpus path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
AUTO, FFT, EXACT, FFT_PCM = 0, 5, 6, 9


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


def _signal(rng, shape, dtype, full_scale=False):
    if dtype == np.int16:
        if full_scale:  # +-32767 in runs of random length ("square-ish noise"): the filter's overshoot saturates
            n = int(np.prod(shape))
            runs = rng.integers(1, 40, size=n)
            sign = np.repeat(np.where(rng.random(n) < 0.5, -32767, 32767), runs)[:n]
            return sign.reshape(shape).astype(np.int16)
        return np.clip(np.rint(rng.standard_normal(shape) * 5000), -32768, 32767).astype(np.int16)
    return np.clip(np.rint(rng.standard_normal(shape) * 2.0 ** 27), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int32)


def _host_stage(oracle, yf, dtype, dither, seed):
    """Float job result [clips, frames, channels] (numpy) -> (integer array, clip count) through oracle.quantize per column."""
    out = np.empty(yf.shape, dtype)
    clips = 0
    for c in range(yf.shape[0]):
        for ch in range(yf.shape[2]):
            q, n = oracle.quantize(yf[c, :, ch], dtype, channel=ch, k0=0, dither=dither, seed=seed)
            out[c, :, ch] = q
            clips += n
    return out, clips


def _as3(a):
    return a[None, :, None] if a.ndim == 1 else (a[None] if a.ndim == 2 else a)


def _check_identity(oracle, plan, x, dither, seed):
    """x: integer numpy array of rank 1-3.  PCM job == float job of the same width + host output stage."""
    import torch
    from soxr_amd import device as dev
    xt = torch.from_numpy(x).cuda()
    xf = xt.float() if x.dtype == np.int16 else xt.double()
    assert xf.stride() == xt.stride()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    y = dev.resample_tensor(plan, xt, kernel=FFT_PCM, dither=dither, dither_seed=seed, clip_counter=counter)
    assert y.dtype == xt.dtype and y.ndim == xt.ndim
    yf = dev.resample_tensor(plan, xf, kernel=FFT)
    assert y.shape == yf.shape
    want, clips = _host_stage(oracle, _as3(yf.cpu().numpy()), x.dtype, dither, seed)
    got = _as3(y.cpu().numpy())
    ndiff = int(np.count_nonzero(got != want))
    print(f"identity {x.dtype} {x.shape} dither={dither} seed={seed}: {ndiff} of {got.size} differ, "
          f"device clips {int(counter.item())} host clips {clips}")
    assert np.array_equal(got, want), (ndiff, got.size)
    assert int(counter.item()) == clips
    return got, clips


RATIOS = [(48000, 44100), (44100, 48000), (44100, 16000), (96000, 48000), (16000, 48000)]


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("quality", ["VHQ", "HQ"])
@pytest.mark.parametrize("in_rate,out_rate", RATIOS)
def test_identity_with_float_engine_mono_and_batch(oracle, in_rate, out_rate, quality, dtype):
    from soxr_amd import device as dev
    rng = np.random.default_rng(in_rate + out_rate + (1 if quality == "HQ" else 0))
    plan = dev.Plan(in_rate, out_rate, quality)
    _check_identity(oracle, plan, _signal(rng, (30011,), dtype), True, 0)
    _check_identity(oracle, plan, _signal(rng, (3, 20001, 1), dtype), True, 12345)
    _check_identity(oracle, plan, _signal(rng, (9001,), dtype), False, 0)


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
@pytest.mark.parametrize("length", [1, 7, 4703, 4704, 4705, 100001])
def test_identity_lengths_and_edges(oracle, length, dtype):
    from soxr_amd import device as dev
    rng = np.random.default_rng(length)
    plan = dev.Plan(48000, 44100, "VHQ")
    for dither, seed in ((True, 0), (True, 77), (False, 0)):
        _check_identity(oracle, plan, _signal(rng, (length,), dtype), dither, seed)


@pytest.mark.parametrize("quality", ["VHQ", "HQ"])
@pytest.mark.parametrize("in_rate,out_rate", RATIOS)
def test_identity_interleaved_int16_pairs(oracle, in_rate, out_rate, quality):
    """[frames, 2] and [frames, 4] int16: one 4-byte (l, r) word per frame; the float job pairs the same channels."""
    from soxr_amd import device as dev
    rng = np.random.default_rng(in_rate * 3 + out_rate)
    plan = dev.Plan(in_rate, out_rate, quality)
    _check_identity(oracle, plan, _signal(rng, (30011, 2), np.int16), True, 5)
    _check_identity(oracle, plan, _signal(rng, (2, 9001, 4), np.int16), False, 0)
    _check_identity(oracle, plan, _signal(rng, (7, 2), np.int16), True, 0)


@pytest.mark.parametrize("shape", [(50001,), (3, 20001, 1), (30011, 2)])
def test_full_scale_input_counts_only_clips_that_exist(oracle, shape):
    """+-32767 square-ish noise: outputs saturate, and the values the kernels convert but do not store (past the end of a
    column, in the last block's staged run) would add to the count if they were counted."""
    from soxr_amd import device as dev
    rng = np.random.default_rng(len(shape))
    for in_rate, out_rate in ((48000, 44100), (16000, 48000)):
        plan = dev.Plan(in_rate, out_rate, "VHQ")
        for dither in (True, False):
            _, clips = _check_identity(oracle, plan, _signal(rng, shape, np.int16, full_scale=True), dither, 3)
            assert clips > 0


@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_identity_ragged_batch(oracle, dtype):
    """dist.RaggedJob (hipsoxr_job_t::clip_table): lengths including 0 and 1, one launch; per-clip out_frames bound the count."""
    import torch
    from soxr_amd import device as dev, dist
    rng = np.random.default_rng(8)
    lengths = [5000, 0, 1, 12345, 7, 4704, 9999]
    for in_rate, out_rate in ((48000, 44100), (44100, 16000)):
        plan = dev.Plan(in_rate, out_rate, "VHQ")
        xs = [_signal(rng, (n,), dtype, full_scale=(dtype == np.int16 and i == 3)) for i, n in enumerate(lengths)]
        ti = [torch.from_numpy(x).cuda() for x in xs]
        tf = [t.float() if dtype == np.int16 else t.double() for t in ti]
        for dither, seed in ((True, 9), (False, 0)):
            counter = torch.zeros(1, dtype=torch.int64, device="cuda")
            job = dist.RaggedJob(plan, ti, kernel=FFT_PCM, dither=dither, dither_seed=seed, clip_counter=counter)
            job.launch()
            jobf = dist.RaggedJob(plan, tf, kernel=FFT)
            jobf.launch()
            torch.cuda.synchronize()
            clips = 0
            for i, (y, yf) in enumerate(zip(job.outputs(), jobf.outputs())):
                assert y.shape[0] == plan.out_len(lengths[i])
                want, n = oracle.quantize(yf.cpu().numpy(), dtype, channel=0, k0=0, dither=dither, seed=seed)
                clips += n
                assert np.array_equal(y.cpu().numpy(), want), (i, lengths[i])
            assert int(counter.item()) == clips
            if dtype == np.int16:
                assert clips > 0


def test_identity_odd_offset_view(oracle):
    """A column that starts on an address that is only 2-byte aligned (and a result that does)."""
    import torch
    from soxr_amd import device as dev
    rng = np.random.default_rng(21)
    plan = dev.Plan(48000, 44100, "VHQ")
    base = torch.from_numpy(_signal(rng, (20001,), np.int16)).cuda()
    for off in (1, 3):
        x = base[off:]
        obuf = torch.zeros(plan.out_len(x.shape[0]) + 8, dtype=torch.int16, device="cuda")
        y = dev.resample_tensor(plan, x, out=obuf[off:off + plan.out_len(x.shape[0])], kernel=FFT_PCM, dither=True, dither_seed=1)
        yf = dev.resample_tensor(plan, base.float()[off:], kernel=FFT)
        want, _ = oracle.quantize(yf.cpu().numpy(), np.int16, channel=0, k0=0, dither=True, seed=1)
        assert np.array_equal(y.cpu().numpy(), want)
        assert not obuf[:off].any() and not obuf[off + y.shape[0]:].any()   # nothing written outside the result


@pytest.mark.parametrize("in_rate,out_rate,quality", [(48000, 44100, "VHQ"), (44100, 48000, "VHQ"), (44100, 16000, "HQ"),
                                                      (96000, 48000, "VHQ"), (16000, 48000, "HQ")])
def test_int16_within_one_lsb_of_exact_engine(in_rate, out_rate, quality):
    import torch
    from soxr_amd import device as dev
    rng = np.random.default_rng(31)
    plan = dev.Plan(in_rate, out_rate, quality)
    for shape in ((200003,), (40001, 2)):
        xt = torch.from_numpy(_signal(rng, shape, np.int16)).cuda()
        for dither in (True, False):
            y = dev.resample_tensor(plan, xt, kernel=FFT_PCM, dither=dither, dither_seed=4).cpu().numpy().astype(np.int32)
            e = dev.resample_tensor(plan, xt, kernel=EXACT, dither=dither, dither_seed=4).cpu().numpy().astype(np.int32)
            d = np.abs(y - e)
            print(f"{in_rate}->{out_rate} {quality} {shape} dither={dither}: max |diff| {d.max()} LSB, "
                  f"share of differing samples {np.count_nonzero(d) / d.size:.3e}")
            assert d.max() <= 1


@pytest.mark.parametrize("in_rate,out_rate,quality,tol", [(48000, 44100, "VHQ", 2e-9), (44100, 48000, "VHQ", 2e-9),
                                                          (44100, 16000, "VHQ", 2e-9), (96000, 48000, "VHQ", 2e-9),
                                                          (16000, 48000, "VHQ", 2e-9), (48000, 44100, "HQ", 1e-6),
                                                          (44100, 16000, "HQ", 1e-6)])
def test_int32_against_float64_reference(oracle, in_rate, out_rate, quality, tol):
    """tol: the float64 instance's own bars (test_fft_engine_float64_instance); + 0.5 LSB for the rounding (0.29 LSB RMS)."""
    import torch
    from soxr_amd import device as dev
    rng = np.random.default_rng(41)
    plan = dev.Plan(in_rate, out_rate, quality)
    x = _signal(rng, (60001,), np.int32)
    y = dev.resample_tensor(plan, torch.from_numpy(x).cuda(), kernel=FFT_PCM).cpu().numpy()
    ref = oracle.resample(x.astype(np.float64), in_rate, out_rate, quality, mode="ref")
    assert y.shape == ref.shape and y.dtype == np.int32
    err = _rms(y.astype(np.float64) - ref)
    print(f"{in_rate}->{out_rate} {quality}: error RMS {err:.3f} LSB, bound {tol * _rms(ref) + 0.5:.3f} (RMS(ref) {_rms(ref):.4g})")
    assert err <= tol * _rms(ref) + 0.5


def test_refusals():
    import torch
    from soxr_amd import device as dev
    rng = np.random.default_rng(51)
    x16 = torch.from_numpy(_signal(rng, (20000,), np.int16)).cuda()
    vhq = dev.Plan(48000, 44100, "VHQ")
    with pytest.raises(RuntimeError, match="int16 / int32"):            # float jobs have KERNEL_FFT
        dev.resample_tensor(vhq, x16.float(), kernel=FFT_PCM)
    with pytest.raises(RuntimeError, match="int16 / int32"):
        dev.resample_tensor(vhq, x16.double(), kernel=FFT_PCM)
    with pytest.raises(RuntimeError, match="HQ/VHQ exact-ratio"):       # MQ: 104 dB stop band
        dev.resample_tensor(dev.Plan(48000, 44100, "MQ"), x16, kernel=FFT_PCM)
    with pytest.raises(RuntimeError, match="HQ/VHQ exact-ratio"):       # interpolated-phase plan
        dev.resample_tensor(dev.Plan(48000, 44101.5, "VHQ"), x16, kernel=FFT_PCM)
    with pytest.raises(RuntimeError, match="unavailable for this plan or layout"):   # a ratio without a schedule
        dev.resample_tensor(dev.Plan(48000, 44000, "VHQ"), x16, kernel=FFT_PCM)
    # layouts outside the three served ones are an error too, never the exact engine: int32 channel pairs,
    # an odd channel count, a strided single column
    x32 = torch.from_numpy(_signal(rng, (20000, 2), np.int32)).cuda()
    with pytest.raises(RuntimeError, match="unavailable for this plan or layout"):
        dev.resample_tensor(vhq, x32, kernel=FFT_PCM)
    x3 = torch.from_numpy(_signal(rng, (20000, 3), np.int16)).cuda()
    with pytest.raises(RuntimeError, match="unavailable for this plan or layout"):
        dev.resample_tensor(vhq, x3, kernel=FFT_PCM)
    with pytest.raises(RuntimeError, match="unavailable for this plan or layout"):
        dev.resample_tensor(vhq, x3[:, 0], kernel=FFT_PCM)
    # what was pinned before stays: integers and the float selector
    with pytest.raises(RuntimeError, match="FFT engine needs"):
        dev.resample_tensor(vhq, x16, kernel=FFT)


@pytest.mark.parametrize("shape", [(30011,), (3, 20001, 1), (30011, 2)])
def test_auto_is_still_the_exact_engine_and_pcm_is_deterministic(shape):
    import torch
    from soxr_amd import device as dev
    rng = np.random.default_rng(61)
    plan = dev.Plan(48000, 44100, "VHQ")
    for dtype in (np.int16, np.int32):
        xt = torch.from_numpy(_signal(rng, shape, dtype)).cuda()
        for dither in (True, False):
            a = dev.resample_tensor(plan, xt, kernel=AUTO, dither=dither)
            e = dev.resample_tensor(plan, xt, kernel=EXACT, dither=dither)
            assert torch.equal(a, e)
        if dtype == np.int32 and len(shape) == 2:
            continue                                         # (int32 channel pairs: not served, test_refusals)
        p1 = dev.resample_tensor(plan, xt, kernel=FFT_PCM, dither=True, dither_seed=2)
        p2 = dev.resample_tensor(plan, xt, kernel=FFT_PCM, dither=True, dither_seed=2)
        assert torch.equal(p1, p2)
        p3 = dev.resample_tensor(plan, xt, kernel=FFT_PCM, dither=True, dither_seed=3)
        assert (dtype == np.int32) == bool(torch.equal(p1, p3))   # the seed matters where there is dither: int16


def test_prepared_job_takes_the_selector_and_seed():
    import torch
    from soxr_amd import device as dev
    rng = np.random.default_rng(71)
    plan = dev.Plan(48000, 44100, "VHQ")
    xt = torch.from_numpy(_signal(rng, (30011,), np.int16)).cuda()
    out = torch.empty(plan.out_len(30011), dtype=torch.int16, device="cuda")
    dev.PreparedJob(plan, xt, out, kernel=FFT_PCM, dither=True, dither_seed=6).launch()
    assert torch.equal(out, dev.resample_tensor(plan, xt, kernel=FFT_PCM, dither=True, dither_seed=6))


@pytest.mark.parametrize("in_rate,out_rate", [(48000, 44100), (44100, 16000)])
def test_corpus_path(in_rate, out_rate):
    """dist.resample_batch on int16 numpy clips of unequal length == clip-by-clip resample_tensor, same selector.
    (Sizes at which the batch and a single clip take the same block size: the float engine's size rules move to larger
    blocks from ~480 block pairs per launch, and another block size is another rounding of the same 1e-6-class result.)"""
    import torch
    from soxr_amd import device as dev, dist
    rng = np.random.default_rng(81)
    clips = [_signal(rng, (n,), np.int16) for n in (12000, 1, 7001, 0, 20011, 4704)]
    got = dist.resample_batch(clips, in_rate, out_rate, quality="VHQ", devices=[0], kernel=FFT_PCM)
    plan = dev.Plan(in_rate, out_rate, "VHQ")
    for x, y in zip(clips, got):
        assert isinstance(y, np.ndarray) and y.dtype == np.int16 and y.shape == (plan.out_len(len(x)),)
        if len(x):
            one = dev.resample_tensor(plan, torch.from_numpy(x).cuda(), kernel=FFT_PCM, dither=True).cpu().numpy()
            assert np.array_equal(y, one)
