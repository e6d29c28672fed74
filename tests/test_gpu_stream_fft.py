"""Device streams on the frequency-domain engine: TensorStream(engine="fft") / HIPSOXR_STREAM_FFT.

Every call returns exactly the frames the default (canonical-order) stream returns; the values are the frequency-domain
engine's — 1e-6-class against the oracle's float64 direct form, globally AND around every chunk seam (the bars and the
normalisation: tests/stream_fft_checks.py); integer streams equal the float stream of their arithmetic width pushed
through the host restatement of the output stage, sample for sample, across seams; nothing is written outside the result;
what the engine cannot serve is refused by name; the default stream is untouched."""
import ctypes as C
import random

import numpy as np
import pytest

import stream_fft_checks as sc

pytestmark = pytest.mark.gpu
FIXED_PLAN = [17, 0, 4410, 48000, 1, 480000, 7]
TOTAL = sum(FIXED_PLAN)
RATES = [(48000, 44100), (44100, 48000), (44100, 16000), (48000, 16000), (96000, 48000)]


def _plans(seed):
    return [("fixed", FIXED_PLAN), ("whole", [TOTAL]), ("random", sc.random_plan(random.Random(seed), TOTAL))]


# ---- 1. counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_rate,out_rate,quality,ch,dtype", [
    (48000, 44100, "VHQ", 1, np.float32), (44100, 48000, "HQ", 2, np.float32), (44100, 16000, "VHQ", 8, np.float32),
    (48000, 16000, "HQ", 3, np.float64), (96000, 48000, "VHQ", 1, np.int16), (44100, 16000, "HQ", 2, np.int16),
    (48000, 44100, "VHQ", 1, np.int32)])
def test_counts_and_delay_equal_the_default_stream(in_rate, out_rate, quality, ch, dtype):
    from soxr_amd import device as dev
    rng = np.random.default_rng(1)
    x = sc.signal(rng, TOTAL, ch, dtype)
    plan = dev.Plan(in_rate, out_rate, quality)
    for name, sizes in _plans(in_rate + ch):
        ts = dev.TensorStream(in_rate, out_rate, ch, dtype=sc.torch_dtype(dtype), quality=quality, engine="fft")
        tw = dev.TensorStream(in_rate, out_rate, ch, dtype=sc.torch_dtype(dtype), quality=quality)
        outs = sc.feed(ts, x, sizes, twin=tw)
        assert sum(len(o) for o in outs) == plan.out_len(TOTAL), name
        assert b"fft" in dev._n.lib.hipsoxr_stream_engine(ts._h)


# ---- 2. values, float -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
@pytest.mark.parametrize("quality", ["VHQ", "HQ"])
@pytest.mark.parametrize("in_rate,out_rate", RATES)
def test_float_values_globally_and_at_every_seam(oracle, in_rate, out_rate, quality, ch):
    """mono: k_fft_pair2; 2 and 8 channels: channel pairs; 3 channels: strided columns.  float32 and float64 on the same
    (float32-representable) values, three chunk plans each, one reference."""
    from soxr_amd import device as dev
    rng = np.random.default_rng(in_rate + out_rate + ch)
    x32 = sc.signal(rng, TOTAL, ch, np.float32)
    ref = oracle.resample(x32.astype(np.float64), in_rate, out_rate, quality, mode="ref")
    taps = dev.Plan(in_rate, out_rate, quality).taps
    for dtype in (np.float32, np.float64):
        for name, sizes in _plans(in_rate + out_rate + ch):
            ts = dev.TensorStream(in_rate, out_rate, ch, dtype=sc.torch_dtype(dtype), quality=quality, engine="fft")
            outs = sc.feed(ts, x32.astype(dtype), sizes)
            sc.check_values(outs, ref, taps, sc.tolerance(dtype, quality),
                            f"{in_rate}->{out_rate} {quality} ch={ch} {np.dtype(dtype).name} {name}")


# ---- 3. values, integer ---------------------------------------------------------------------------------------------
INT_PLAN = [17, 0, 4410, 48000, 1, 100003, 7]


@pytest.mark.parametrize("in_rate,out_rate,quality", [(48000, 44100, "VHQ"), (44100, 48000, "HQ"), (44100, 16000, "VHQ"),
                                                      (96000, 48000, "HQ"), (16000, 48000, "VHQ")])
@pytest.mark.parametrize("dtype,ch", [(np.int16, 1), (np.int16, 2), (np.int16, 8), (np.int32, 1)])
def test_integer_streams_equal_float_stream_plus_output_stage(oracle, in_rate, out_rate, quality, dtype, ch):
    from soxr_amd import device as dev
    rng = np.random.default_rng(in_rate + ch)
    n = sum(INT_PLAN)
    what = f"{in_rate}->{out_rate} {quality} {np.dtype(dtype).name} ch={ch}"
    sc.check_integer_identity(oracle, dev, in_rate, out_rate, quality, sc.signal(rng, n, ch, dtype), INT_PLAN, True, 12345, what + " dither")
    sc.check_integer_identity(oracle, dev, in_rate, out_rate, quality, sc.signal(rng, n, ch, dtype), INT_PLAN, False, 0, what + " no dither")
    if dtype == np.int16:  # full scale: clips exist, and only stored samples count — at every seam too
        clips = sc.check_integer_identity(oracle, dev, in_rate, out_rate, quality, sc.signal(rng, n, ch, dtype, full_scale=True),
                                          sc.random_plan(random.Random(ch), n, 60000), True, 3, what + " full scale")
        assert clips > 0


# ---- 4. nothing outside the result ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,ch,off", [(np.int16, 1, 1), (np.int16, 1, 3), (np.int16, 2, 1), (np.int16, 2, 3), (np.int16, 8, 1),
                                          (np.float32, 1, 1), (np.float32, 1, 3), (np.float32, 2, 1), (np.float32, 3, 1),
                                          (np.float64, 1, 1), (np.float64, 2, 1), (np.float64, 3, 1), (np.int32, 1, 1)])
@pytest.mark.parametrize("in_rate,out_rate", [(48000, 44100), (44100, 16000), (16000, 48000)])
def test_nothing_is_written_outside_the_result(in_rate, out_rate, dtype, ch, off):
    """The C entry with olen = the exact count, the result in the middle of a poisoned buffer at frame offset `off` (int16
    mono: odd element offsets; int16 stereo: 4-byte aligned, not 16): every element outside [out, out + n) keeps the poison
    after every call.  Chunk sizes are odd primes and the like, so a chunk's first output falls mid-run and mid-granule."""
    import torch
    from soxr_amd import device as dev, _native as _n
    rng = np.random.default_rng(off)
    sizes = [4411, 10007, 1, 48001, 23, 20011, 6007]
    x = sc.signal(rng, sum(sizes), ch, dtype)
    xt = torch.from_numpy(x).cuda()
    tdt = sc.torch_dtype(dtype)
    ts = dev.TensorStream(in_rate, out_rate, ch, dtype=tdt, quality="VHQ", engine="fft")
    tw = dev.TensorStream(in_rate, out_rate, ch, dtype=tdt, quality="VHQ")
    fn, done = _n.lib.hipsoxr_stream_process_device, C.c_size_t(0)
    stream = torch.cuda.current_stream().cuda_stream
    poison = 0x5A5A if dtype == np.int16 else 0x5A5A5A5A if dtype == np.int32 else float("inf")
    es, pos, guard = x.itemsize, 0, 4096
    got = []
    for i, n_in in enumerate(sizes):
        last = i == len(sizes) - 1
        chunk = xt[pos:pos + n_in].contiguous()
        pos += n_in
        want = int(tw.resample_chunk(chunk, last=last).shape[0])  # the default stream's count for this call
        buf = torch.full(((guard + off + want + guard) * ch,), poison, dtype=tdt, device="cuda")
        optr = buf.data_ptr() + (guard + off) * ch * es
        _n.check(fn(ts._h, chunk.data_ptr(), n_in, optr, want, C.byref(done), stream))
        n = done.value
        if last and n < want:  # flush: the rest, with the exact count again
            _n.check(fn(ts._h, None, 0, optr + n * ch * es, want - n, C.byref(done), stream))
            n += done.value
        assert n == want, (i, n, want)
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        lo, hi = (guard + off) * ch, (guard + off + want) * ch
        assert np.all(b[:lo] == poison) and np.all(b[hi:] == poison), (i, n_in, want, np.flatnonzero(b[:lo] != poison)[:8],
                                                                       np.flatnonzero(b[hi:] != poison)[:8])
        if want and dtype in (np.float32, np.float64):
            assert np.all(np.isfinite(b[lo:hi])), i  # ... and every element of the result WAS written
        got.append(b[lo:hi].reshape((want, ch) if ch > 1 else (want,)))
    # the same frames as the tensor surface returns
    t2 = dev.TensorStream(in_rate, out_rate, ch, dtype=tdt, quality="VHQ", engine="fft")
    assert np.array_equal(np.concatenate(got), np.concatenate(sc.feed(t2, x, sizes)))


# ---- 5. state -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,ch", [(np.float32, 1), (np.float32, 2), (np.int16, 2), (np.float64, 3)])
def test_clear_gives_a_fresh_stream(dtype, ch):
    """A result is a function of the signal and its cut into chunks alone — not of what the ring held or when it was
    compacted (engine.cpp first_needed: the ring keeps a block's whole lead-in): bit for bit after clear()."""
    from soxr_amd import device as dev
    rng = np.random.default_rng(5)
    sizes = [30000, 7, 100000, 12345, 50000]
    x = sc.signal(rng, sum(sizes), ch, dtype)
    ts = dev.TensorStream(48000, 44100, ch, dtype=sc.torch_dtype(dtype), quality="VHQ", engine="fft")
    sc.feed(ts, sc.signal(rng, 77777, ch, dtype), [70000, 7777])
    ts.clear()
    assert ts.delay() == 0.0
    a = np.concatenate(sc.feed(ts, x, sizes))
    fresh = dev.TensorStream(48000, 44100, ch, dtype=sc.torch_dtype(dtype), quality="VHQ", engine="fft")
    assert np.array_equal(a, np.concatenate(sc.feed(fresh, x, sizes)))
    if np.dtype(dtype) == np.int16:
        assert ts.num_clips() == fresh.num_clips()


def test_small_first_chunk_inherited_host_ring_then_large(oracle, soxr):
    """A finished small-chunk host stream hands its ring (pinned host memory) to the pool; the next stream inherits it and
    moves it to the device at its first device call."""
    from soxr_amd import device as dev
    rng = np.random.default_rng(6)
    rs = soxr.ResampleStream(48000, 44100, 1, dtype="float32", quality="VHQ")
    rs.resample_chunk(np.zeros(441, np.float32))
    rs.resample_chunk(np.zeros(441, np.float32), last=True)
    del rs
    sizes = [100, 333, 200000, 5, 90000]
    x = sc.signal(rng, sum(sizes), 1, np.float32)
    ts = dev.TensorStream(48000, 44100, 1, quality="VHQ", engine="fft")
    tw = dev.TensorStream(48000, 44100, 1, quality="VHQ")
    outs = sc.feed(ts, x, sizes, twin=tw)
    ref = oracle.resample(x.astype(np.float64), 48000, 44100, "VHQ", mode="ref")
    sc.check_values(outs, ref, dev.Plan(48000, 44100, "VHQ").taps, 1e-6, "inherited host ring")


@pytest.mark.parametrize("sizes", [[50000, 0], [123457], [0], [1], [3, 0]])
def test_empty_final_call_and_last_on_the_first_call(oracle, sizes):
    from soxr_amd import device as dev
    rng = np.random.default_rng(7)
    for ch, dtype in ((1, np.float32), (2, np.float32), (1, np.int16)):
        x = sc.signal(rng, sum(sizes), ch, dtype)
        ts = dev.TensorStream(44100, 16000, ch, dtype=sc.torch_dtype(dtype), quality="HQ", engine="fft")
        tw = dev.TensorStream(44100, 16000, ch, dtype=sc.torch_dtype(dtype), quality="HQ")
        outs = sc.feed(ts, x, sizes, twin=tw)
        if dtype == np.float32 and sum(sizes) > 100:
            ref = oracle.resample(x.astype(np.float64), 44100, 16000, "HQ", mode="ref")
            sc.check_values(outs, ref, dev.Plan(44100, 16000, "HQ").taps, 1e-6, f"sizes {sizes} ch={ch}")
        with pytest.raises(RuntimeError, match="Input after last input"):
            ts.resample_chunk(__import__("torch").zeros((1, ch) if ch > 1 else 1, dtype=sc.torch_dtype(dtype), device="cuda"))


# ---- 6. refusals ----------------------------------------------------------------------------------------------------
def test_creation_refuses_by_name_what_the_engine_cannot_serve():
    import torch
    from soxr_amd import device as dev, _native as _n

    def refused(match, *a, **kw):
        with pytest.raises(RuntimeError, match=match) as e:
            dev.TensorStream(*a, engine="fft", **kw)
        assert "STREAM_FFT" in str(e.value)

    refused("variable-rate", 48000, 44100, 1, vr=True)
    refused("exact polyphase bank", 48000, 44101.5, 1, quality="VHQ")
    for q in ("MQ", "LQ", "QQ"):
        refused("HQ and VHQ", 48000, 44100, 1, quality=q)
    refused("int32 streams", 48000, 44100, 2, dtype=torch.int32, quality="VHQ")
    refused("int16 streams", 48000, 44100, 3, dtype=torch.int16, quality="VHQ")
    for dt in (torch.float32, torch.float64, torch.int16, torch.int32):  # 3/8: an exact bank, but no paired-kernel schedule
        refused("schedule table", 32000, 12000, 1, dtype=dt, quality="VHQ")
    # flags and layouts the Python surface does not expose: the C entry
    for io, flags, match in ((_n.FLOAT32_S, _n.STREAM_FFT, b"split"), (_n.INT16_S, _n.STREAM_FFT, b"split"),
                             (_n.FLOAT32_I, _n.STREAM_FFT | _n.DEFER, b"DEFER"), (_n.FLOAT32_I, _n.STREAM_FFT | _n.RESIDENT, b"RESIDENT"),
                             (_n.FLOAT32_I, _n.STREAM_FFT | _n.AUTO_RESIDENT, b"AUTO_RESIDENT")):
        h = C.c_void_p()
        err = _n.lib.hipsoxr_stream_create(48000.0, 44100.0, 2, io, _n.VHQ, flags, C.byref(h))
        assert err and match in err and b"STREAM_FFT" in err and not h.value, err
    with pytest.raises(ValueError):
        dev.TensorStream(48000, 44100, 1, engine="fast")


def test_host_pointer_grouped_and_ratio_calls_are_refused_on_a_flagged_handle():
    import torch
    from soxr_amd import device as dev, _native as _n
    ts = dev.TensorStream(48000, 44100, 1, quality="VHQ", engine="fft")
    x = np.zeros(1000, np.float32)
    y = np.zeros(2000, np.float32)
    done = C.c_size_t(0)
    err = _n.lib.hipsoxr_stream_process(ts._h, x.ctypes.data, 1000, y.ctypes.data, 2000, C.byref(done))
    assert err and b"STREAM_FFT" in err and done.value == 0
    xt, yt = torch.zeros(1000, device="cuda"), torch.zeros(2000, device="cuda")
    other = dev.TensorStream(48000, 44100, 1, quality="VHQ")
    for hs in ([ts], [other, ts]):
        n = len(hs)
        handles = (C.c_void_p * n)(*[s._h.value for s in hs])
        ins, outs = np.full(n, xt.data_ptr(), np.uint64), np.full(n, yt.data_ptr(), np.uint64)
        ilens, olens, dones = np.full(n, 1000, np.uint64), np.full(n, 2000, np.uint64), np.zeros(n, np.uint64)
        err = _n.lib.hipsoxr_streams_process_device(handles, n, ins.ctypes.data, ilens.ctypes.data, outs.ctypes.data, olens.ctypes.data,
                                                    dones.ctypes.data, torch.cuda.current_stream().cuda_stream)
        assert err and b"STREAM_FFT" in err and not dones.any()
    with pytest.raises(RuntimeError, match="variable-rate"):
        ts.set_io_ratio(48000, 40000)
    # ... and the handle still works
    assert ts.resample_chunk(xt, last=True).shape[0] == dev.Plan(48000, 44100, "VHQ").out_len(1000)


def test_public_whole_signal_path_still_refuses_a_window():
    import torch
    from soxr_amd import device as dev
    plan = dev.Plan(48000, 44100, "VHQ")
    x, y = torch.zeros(48000, device="cuda"), torch.zeros(44100, device="cuda")
    with pytest.raises(RuntimeError, match="whole-signal"):
        plan.run(x.data_ptr(), y.data_ptr(), dev._n.F32, 1, 1, 48000, 1000, (0, 1, 1), (0, 1, 1), kernel=dev.KERNEL_FFT, out_k0=147)
    with pytest.raises(RuntimeError, match="whole-signal"):
        plan.run(x.data_ptr(), y.data_ptr(), dev._n.F32, 1, 1, 40000, 1000, (0, 1, 1), (0, 1, 1), kernel=dev.KERNEL_FFT, in_abs0=160)


# ---- 7. the default is untouched ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,ch", [(np.float32, 1), (np.int16, 2)])
def test_default_stream_is_still_the_canonical_order_bit_for_bit(oracle, dtype, ch):
    from soxr_amd import device as dev
    rng = np.random.default_rng(9)
    x = sc.signal(rng, TOTAL, ch, dtype)
    ts = dev.TensorStream(48000, 44100, ch, dtype=sc.torch_dtype(dtype), quality="VHQ")
    assert ts.engine == "exact"
    y = np.concatenate(sc.feed(ts, x, FIXED_PLAN))
    assert np.array_equal(y, oracle.resample(x, 48000, 44100, "VHQ", mode="port"))
